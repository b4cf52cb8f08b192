"""Rule sets over the whole space of second, minute and hour masks: the
popcounts nS, nM and nH are the mixed-radix digits of the closed-form writer
(cg_write.h coop_cf), and the bit patterns feed its rank tables, its
arithmetic-progression test, the per-lane seek and the partial-mask ranks of
the profile (cg_time.h tod_rank).  A helper module, not a test:
tests/test_mask_cases.py checks on the CPU that the sets hold what they
promise and tests/test_gpu_masks.py runs them on the GPU.

Every mask is written as a comma list ("3,17,18,40"), so that the product
parser and the oracle's own parser both read it.

Empty second and minute lists are left out on purpose: the reference's Next
then takes about 10^8 steps per call before it reaches its five-year limit,
which is a time sink on both sides and no kernel edge.
"""
import numpy as np

TOP = {"second": 59, "minute": 59, "hour": 23}
LEVELS = ("second", "minute", "hour")


def _list(vals):
    return ",".join(str(int(v)) for v in sorted(vals))


def _subset(rng, n, lo, hi):
    """a uniform random n-subset of lo..hi as a comma list"""
    return _list(lo + rng.choice(hi - lo + 1, size=n, replace=False))


def _day_fields(rng, form):
    """dom, month and dow of one of the four day forms (month '*')"""
    dom = _subset(rng, int(rng.integers(25, 31)), 1, 31)
    dow = _subset(rng, int(rng.integers(5, 7)), 0, 6)
    return (("*", "*"), (dom, "*"), ("?", dow), (dom, dow))[form]


def stratified(n, seed, sparse=False):
    """n rules; rule i has nS = 1 + i % 60 second bits, nM = 1 + 7i % 60 minute
    bits and nH = 1 + 5i % 24 hour bits, each a uniform random subset of that
    size (n = 360: 120 distinct triples, every value of each radix).  The day
    fields cycle through '* * *', a dom list with dow '*', '?' with a dow list,
    and both lists (the OR rule); one rule in five has a random month subset.
    sparse caps nS at 3, for horizons longer than a day."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        nS, nM, nH = 1 + i % 60, 1 + 7 * i % 60, 1 + 5 * i % 24
        if sparse:
            nS = 1 + (nS - 1) % 3
        sec, mnt, hour = _subset(rng, nS, 0, 59), _subset(rng, nM, 0, 59), _subset(rng, nH, 0, 23)
        dom, dow = _day_fields(rng, i % 4)
        month = _subset(rng, int(rng.integers(9, 12)), 1, 12) if i % 5 == 0 else "*"
        out.append(f"{sec} {mnt} {hour} {dom} {month} {dow}")
    return out


def radices(i):
    """(nS, nM, nH) of rule i of stratified(.., sparse=False)"""
    return 1 + i % 60, 1 + 7 * i % 60, 1 + 5 * i % 24


# ---------------------------------------------------------------- extremes
def _ap(first, step, top):
    return list(range(first, top + 1, step))


def level_patterns(level):
    """{name: field text} of one level's edge masks (top = 59, or 23 for hours).
    The patterns about bits 31 and 32 apply to the 60-bit levels only; the
    hour level has its own two lists instead."""
    top = TOP[level]
    full = set(range(top + 1))
    p = {"bit0": "0", "top": str(top), "0+top": f"0,{top}"}
    holes = (0, 31, 32, 59) if top == 59 else (0, 11, 12, 23)
    for h in holes:
        p[f"all-but-{h}"] = _list(full - {h})
    p["even"] = _list(range(0, top + 1, 2))
    p["odd"] = _list(range(1, top + 1, 2))
    p["ap-first>=step"] = f"7-{top}/5"
    p["ap-step-not-dividing"] = "*/7"
    ap = _ap(3, 4, top)
    p["ap-minus-one"] = _list(set(ap) - {ap[len(ap) // 2]})
    p["ap-plus-one"] = _list(set(ap) | {ap[1] + 1})
    if top == 59:
        p["31+32"] = "31,32"
        p["bits32-59"] = _list(range(32, 60))
        p["bits0-31"] = _list(range(0, 32))
    else:
        p["1,2,4,8,16"] = "1,2,4,8,16"
        p["0,23"] = "0,23"
    return p


DAY_PATTERNS = {"dom-1,2,4,8,16,31": "1,2,4,8,16,31 * ?", "dom-31": "31 * ?", "dow-Mon,Tue,Thu": "? * Mon,Tue,Thu"}
NEVER = {"empty-hour": "0 0 , * * *", "empty-dom": "0 0 0 , * *", "empty-month": "0 0 0 * , *"}


def _table_mask(rng, level):
    """a random mask of 3..7 bits that is no arithmetic progression (a one-bit
    pattern with two of them fires at most 49 times a day: a tiny run)"""
    top = TOP[level]
    while True:
        v = sorted((rng.choice(top + 1, size=int(rng.integers(3, 8)), replace=False)).tolist())
        if len({b - a for a, b in zip(v, v[1:])}) > 1:
            return _list(v)


def extremes_named():
    """[(name, spec)]: every pattern of every level with the other levels '*'
    ('<level>/<pattern>/star') and with the other levels a random table mask
    ('.../table'), the day-field patterns the same way, and the three rules
    that never fire."""
    rng = np.random.default_rng(0xE57)
    out = []
    for k, level in enumerate(LEVELS):
        for name, text in level_patterns(level).items():
            for other in ("star", "table"):
                f = ["*" if other == "star" else _table_mask(rng, lv) for lv in LEVELS]
                f[k] = text
                out.append((f"{level}/{name}/{other}", " ".join(f) + " * * *"))
    for name, days in DAY_PATTERNS.items():
        out.append((f"day/{name}/star", "* * * " + days))
        out.append((f"day/{name}/table", " ".join(_table_mask(rng, lv) for lv in LEVELS) + " " + days))
    out += [(f"never/{name}", spec) for name, spec in NEVER.items()]
    return out


def extremes():
    return [s for _, s in extremes_named()]


def day_extremes(sparse=False):
    """The day-field patterns and the never-firing rules of extremes().
    sparse: the '* * *' times of day become '*/20 * *' (three second bits, as
    in stratified(sparse=True)): over 40 days 'Mon,Tue,Thu' alone otherwise
    fires 1.5 M times, all of them in one thread of the oracle."""
    out = [(n, s) for n, s in extremes_named() if n.startswith(("day/", "never/"))]
    return [("*/20" + s[1:]) if sparse and n.endswith("/star") else s for n, s in out]


# --------------------------------------------------------------- junk bits
# bits the reference never looks at, per column (bit 63, the star bit, stays)
JUNK = {"second": (60, 61, 62), "minute": (60, 61, 62), "hour": tuple(range(24, 63)),
        "dom": (0,) + tuple(range(32, 63)), "month": (0,) + tuple(range(13, 63)), "dow": tuple(range(7, 63))}
COLUMNS = ("second", "minute", "hour", "dom", "month", "dow")


def junk_mask(column):
    return sum(1 << b for b in JUNK[column])


def junk_bits(masks, seed):
    """masks: the six clean uint64 columns (second .. dow).  The same columns
    with random bits set where the reference never looks."""
    rng = np.random.default_rng(seed)
    out = []
    for name, col in zip(COLUMNS, masks):
        col = np.asarray(col, dtype=np.uint64)
        noise = rng.integers(0, 1 << 63, col.shape, dtype=np.uint64) & np.uint64(junk_mask(name))
        out.append(col | noise)
    return out


def soa_columns(specs):
    """the six clean uint64 columns of specs, parsed by the product"""
    from cronsun_amd import cron
    s = [cron.Parse(x) for x in specs]
    return [np.array([getattr(x, f) for x in s], dtype=np.uint64)
            for f in ("Second", "Minute", "Hour", "Dom", "Month", "Dow")]
