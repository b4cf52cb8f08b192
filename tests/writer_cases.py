"""Constructed rule sets for the closed-form writer (k_write_cf, cg_write.h):
runs of a known form placed at chosen output positions.  A helper module, not
a test: tests/test_writer_cases.py checks the sets on the CPU and
tests/test_gpu_writer.py runs them on the GPU.

A rule's fire count in a window does not depend on its neighbours, so every
builder asks the oracle's count pass (O.expand_batch(..., with_times=False))
once per distinct spec and places runs by adding counts up; the offsets of a
case are the running sum of those counts.  Filler rules with an exact number
of fires sit in front of a run and shift it.

A rule's form is a property of its masks (spec_form), not of the kernel:

  every   @every Ns
  tiny    fewer than 64 fires in the window
  table   the second, minute or hour set, or the set of matching days of the
          window, is not an arithmetic progression
  linear  every level is one, and on consecutive days the fires are equally
          spaced (the times of day are equally spaced around the 24-h circle
          and the matching days are consecutive, or there is one time of day
          and the matching days are a progression)
  affine  every level is one, with more than one spacing

A spec confined to one hour ("*/2 * 1 * * *") is therefore affine: its spacing
breaks at the end of the hour.
"""
import datetime
import functools
from collections import namedtuple

import numpy as np

import oracle_lib as O
from common import oracle_parse_all, oracle_zone
from cronsun_amd import synth

T0 = synth.T0_2026  # a UTC midnight (a Monday)
DAY = 86400
OFF_MIDNIGHT = 7 * 3600 + 13 * 60 + 37
LORD_HOWE = "Australia/Lord_Howe"
LORD_HOWE_T0 = 1775314800 - DAY // 2 - 17  # 12 h before its 2026-04-04 15:00 Z transition

FORMS = ("linear", "affine", "table", "every", "tiny", "empty")
LONG_FORMS = ("linear", "affine", "table", "every")
SLICE = 2048  # events per position slice (capacity below 2^31)

RESIDUES = (0, 1, 31, 32, 33, 62, 63)
SWEEP_L = (1, 2, 63, 64, 65, 127, 128, 129, 511, 512, 513, 575, 576, 577, 639, 640, 641,
           2047, 2048, 2049, 2111, 2112, 2113)
FIB = "1,2,3,5,8,13,21,34,55"

# one rule per row: its form, fires, start position mod 64, length class
# (index into LENGTH_CLASSES), whether a 2048-boundary falls strictly inside
# the run / exactly on its start
Ledger = namedtuple("Ledger", "form count residue length_class cut_inside cut_at_start")
LENGTH_CLASSES = ("0", "1-63", "64-639", "640-2047", "2048-")
Case = namedtuple("Case", "name specs zone t0 t1 off ledger")


# ------------------------------------------------------------------ forms
def bits(mask):
    return [i for i in range(63) if (mask >> i) & 1]


def is_ap(mask):
    """Is the set of bit positions of mask an arithmetic progression?
    (the empty set and single values count)"""
    p = bits(mask)
    return all(p[i + 1] - p[i] == p[1] - p[0] for i in range(1, len(p) - 1))


def _utc_date(t):
    return datetime.datetime.fromtimestamp(t, datetime.timezone.utc).date()


def window_days(zone, t0, t1):
    """the local dates that (t0, t1] touches"""
    z = oracle_zone(zone)
    first = _utc_date(t0 + 1 + z.lookup(t0 + 1)[0])
    last = _utc_date(t1 + z.lookup(t1)[0])
    return [first + datetime.timedelta(days=i) for i in range((last - first).days + 1)]


def day_mask(s, days):
    """bit i: days[i] matches the spec's day fields (spec.go dayMatches)"""
    star = 1 << 63
    m = 0
    for i, d in enumerate(days):
        dom = (s.spec.dom >> d.day) & 1
        dow = (s.spec.dow >> ((d.weekday() + 1) % 7)) & 1
        ok = (dom and dow) if (s.spec.dom & star or s.spec.dow & star) else (dom or dow)
        if ok and (s.spec.month >> d.month) & 1:
            m |= 1 << i
    return m


_form_cache = {}


def spec_form(spec, count, zone, t0, t1):
    if count == 0:
        return "empty"
    if count < 64:
        return "tiny"
    key = (spec, zone, t0, t1)
    if key not in _form_cache:
        _form_cache[key] = _long_form(O.parse(spec)[0], window_days(zone, t0, t1))
    return _form_cache[key]


def _long_form(s, days):
    if s.kind != 0:
        return "every"
    S, M, H = s.spec.second & (2 ** 60 - 1), s.spec.minute & (2 ** 60 - 1), s.spec.hour & (2 ** 24 - 1)
    D = day_mask(s, days)
    if not (is_ap(S) and is_ap(M) and is_ap(H) and is_ap(D)):
        return "table"
    tod = (3600 * np.array(bits(H))[:, None, None] + 60 * np.array(bits(M))[None, :, None]
           + np.array(bits(S))[None, None, :]).ravel()
    dd = np.diff(bits(D))
    if len(tod) == 1:
        return "linear"  # one fire per matching day, the days a progression
    gaps = np.diff(np.append(tod, tod[0] + DAY))
    return "linear" if (gaps == gaps[0]).all() and (dd == 1).all() else "affine"


# ------------------------------------------------------------ oracle counts
_count_cache = {}


def counts_of(specs, zone, t0, t1):
    """fires of each spec in (t0, t1]: the oracle's count pass, once per distinct spec"""
    new = sorted({s for s in specs if (s, zone, t0, t1) not in _count_cache})
    if new:
        off, _ = O.expand_batch(O.sched_array(oracle_parse_all(new)), t0, t1, oracle_zone(zone), with_times=False)
        for s, n in zip(new, np.diff(off)):
            _count_cache[(s, zone, t0, t1)] = int(n)
    return [_count_cache[(s, zone, t0, t1)] for s in specs]


def make_case(name, specs, zone, t0, t1):
    cnt = np.array(counts_of(specs, zone, t0, t1), dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    return Case(name, list(specs), zone, t0, t1, off, ledger_of(specs, off, zone, t0, t1))


def ledger_of(specs, off, zone, t0, t1):
    cnt = np.diff(off)
    start = off[:-1]
    form = np.array([FORMS.index(spec_form(s, int(n), zone, t0, t1)) for s, n in zip(specs, cnt)], dtype=np.int8)
    lc = np.searchsorted(np.array([1, 64, 640, 2048]), cnt, side="right").astype(np.int8)
    inside = (cnt > 0) & ((off[1:] - 1) // SLICE > start // SLICE)
    at_start = (cnt > 0) & (start % SLICE == 0)
    return Ledger(form, cnt, (start % 64).astype(np.int8), lc, inside, at_start)


def totals(case):
    """rules, events and rules per form of a case (for reports)"""
    per = {f: int((case.ledger.form == i).sum()) for i, f in enumerate(FORMS)}
    return {"rules": len(case.specs), "events": int(case.off[-1]), "forms": per}


def describe(case, rule):
    """a rule of a case, for failure messages"""
    lg = case.ledger
    return (f"rule {rule} '{case.specs[rule]}' form {FORMS[lg.form[rule]]} start {int(case.off[rule])} "
            f"(residue {int(lg.residue[rule])}) fires {int(lg.count[rule])}")


# ---------------------------------------------------------------- fillers
EMPTY = "0 0 0 30 Feb ?"


def filler(k, minute=1, hour=0):
    """k fires (0..60) in a window that holds hour:minute of one local day once"""
    if k == 0:
        return EMPTY
    return f"0-{k - 1} {minute} {hour} * * *" if k > 1 else f"0 {minute} {hour} * * *"


def fillers(k, **kw):
    """rules that fire k times in all, none empty"""
    out = []
    while k > 0:
        out.append(filler(min(k, 60), **kw))
        k -= min(k, 60)
    return out


# ------------------------------------------------------------------ sweep
# Generators confined to hour 1, so that L sets their length: the window
# (T0, T0 + 3600 + L] holds L + 1 seconds of that hour.  None of them can be
# linear (see the module docstring); the linear generators are unconfined and
# fire over the whole window, as @every 1s does.
SWEEP_GENS = ("* * 1 * * *", "*/2 * 1 * * *", "5/10 * 1 * * *", "*/7 * 1 * * *", "* 0-58/2 1 * * *",
              "* * 1-2 * * *", f"{FIB} * 1 * * *", f"* {FIB} 1 * * *", "0-20,22-40 * 1 * * *",
              "*/10 * * * * *", "*/3 * * * * *", "29/30 * * * * *", "@every 1s")


@functools.lru_cache(maxsize=None)
def sweep(L):
    """Every generator at every start residue of RESIDUES, shifted there by
    fillers in hour 0.  About 200 rules; the cost shift of the writer's slices
    stays 6 (E + rules < 2^20)."""
    t0, t1 = T0, T0 + 3600 + L
    n = dict(zip(SWEEP_GENS, counts_of(SWEEP_GENS, "UTC", t0, t1)))
    specs, pos = [], 0
    for g in SWEEP_GENS:
        for r in RESIDUES:
            need = (r - pos) % 64
            specs += fillers(need)
            specs.append(g)
            pos += need + n[g]
    return make_case(f"sweep({L})", specs, "UTC", t0, t1)


# ---------------------------------------------------------------- radices
def _contiguous(n):
    return f"0-{n - 1}"


def _stepped(n, radix, high):
    """n values a, a + k, ..: the largest step k that fits, a = 0 or k - 1"""
    k = max(1, min(radix // n, radix // 2))
    a = k - 1 if high else 0
    return f"{a}-{a + (n - 1) * k}/{k}"


def _holed(n):
    """0..n with one interior value removed: n values, no progression (n >= 4)"""
    gone = 1 + (n * 7) % (n - 1)
    return ",".join(str(v) for v in range(n + 1) if v != gone)


def level_sets(radix):
    """{construction: {size: field text}} for one level"""
    out = {"contiguous": {n: _contiguous(n) for n in range(1, radix + 1)},
           "stepped": {}, "stepped_high": {}, "holed": {n: _holed(n) for n in range(4, radix)}}
    for n in range(1, radix + 1):
        out["stepped"][n] = _stepped(n, radix, False)
        out["stepped_high"][n] = _stepped(n, radix, True)
    return out


DAY_FIELDS = ("* * *", "*/2 * ?", "1,15 * ?", "* * Mon", "* * 1-5")


RADIX_FAMILIES = ("second-ranges+minute", "second-steps+minute", "hour", "day")
RADIX_STARTS = (T0, T0 + OFF_MIDNIGHT)


def radix_rows(family):
    """(days of the window, [(level, construction, size, spec)]) of a family.
    The second-level rules (1440 fires per value) share their two calls with
    the halves of the minute-level family, so that no call is a few heavy
    rules only; the day-level rules have a call of their own."""
    if family.startswith("second"):
        sec, mnt = level_sets(60), level_sets(60)
        # minutes under seconds */10 (a second stride that wraps evenly into the
        # minute); under one second value a stepped minute set can be linear
        minute = [("minute", c, n, f"*/10 {t} * * * *") for c in mnt for n, t in mnt[c].items()]
        minute += [("minute", c, n, f"{s} {mnt[c][n]} * * * *") for s in ("0", "59")
                   for c in ("stepped", "stepped_high") for n in mnt[c]]
        ranges = family == "second-ranges+minute"
        cons = ("contiguous", "holed") if ranges else ("stepped", "stepped_high")
        return 1, ([("second", c, n, f"{t} * * * * *") for c in cons for n, t in sec[c].items()]
                   + minute[0 if ranges else 1::2])
    if family == "hour":
        hour = level_sets(24)
        # */3 */4: 300 fires per hour, so that the call's slices span several
        # blocks (a cost shift above 6) and the digits are stepped, not only seeded
        return 20, [("hour", c, n, f"{s} {t} * * *") for s in ("*/3 */4", "0 0", "30 15", "59 59")
                    for c in hour for n, t in hour[c].items()]
    assert family == "day"
    tods = [f"{x} {m} {h}" for x in ("*/2", "*/10", "0") for m in ("*/10", "*/5", "1-59/7", FIB, "0")
            for h in ("*", "0-22", "9-17", "1/2")]
    return 20, [("day", d, 0, f"{tod} {d}") for d in DAY_FIELDS for tod in tods]


def _dealt(rows, cnt):
    """rows reordered so that every 64 consecutive rules hold about the same
    number of fires (the oracle hands its threads 64 rules at a time)"""
    order = sorted(range(len(rows)), key=lambda i: -cnt[i])
    piles = -(-len(rows) // 64)
    return [rows[i] for k in range(piles) for i in order[k::piles]]


@functools.lru_cache(maxsize=None)
def radix_case(family, start):
    """(case, tags) of one family from one start, tags[i] = (level,
    construction, size) of rule i.  Rules with fewer than 64 fires in the
    window are left out."""
    days, rows = radix_rows(family)
    t0, t1 = start, start + days * DAY
    cnt = counts_of([r[3] for r in rows], "UTC", t0, t1)
    keep = _dealt([r for r, n in zip(rows, cnt) if n >= 64], [n for n in cnt if n >= 64])
    case = make_case(f"radices {family} +{start - T0}s", [r[3] for r in keep], "UTC", t0, t1)
    return case, [r[:3] for r in keep]


def radices():
    """every family from the midnight T0 and from T0 + 7:13:37 (UTC)"""
    return [radix_case(f, s) for s in RADIX_STARTS for f in RADIX_FAMILIES]


# ----------------------------------------------------------------- layout
DENSE = ("* * * * * *", "*/2 * * * * *", "5/10 * * * * *", "*/7 * * * * *", "0-29 * * * * *",
         "* */2 * * * *", f"{FIB} * * * * *", "@every 1s", "@every 2s", "@every 7s",
         f"* {FIB} * * * *", "* * 9-17 * * *", "* * 0-22 * * *", "*/3 */7 1/2 * * *",
         "10-40/3 * * * * *", "* * * * * 1-5", "58-59 * * * * *", "0/15 * * * * *", "* 0-58 * * * *",
         "*/59 * * * * *", "0 * * * * *", "*/20 * * * * *", "0-20,22-40 * * * * *")
# smaller and smaller rules that close the gap to a requested E
GAP_MENU = ("*/2 * * * * *", "5/10 * * * * *", "0 * * * * *", "0 */5 * * * *", "0 0 * * * *")
SPECIAL_LENGTHS = tuple(b + d for b in (64, 576, 2048) for d in (-1, 0, 1))


def special_length_spec(target, holed):
    """A rule with target fires in a 24-h UTC window from a midnight: a product
    of set sizes nS * nM * nH (contiguous sets, or with `holed` the second set
    with one interior value removed), else an @every period; None if neither
    exists."""
    best = None
    for nh in range(1, 25):
        for nm in range(1, 61):
            ns, rem = divmod(target, nh * nm)
            if rem == 0 and (4 if holed else 1) <= ns <= (59 if holed else 60):
                if best is None or ns > best[0]:
                    best = (ns, nm, nh)
    if best:
        ns, nm, nh = best
        return f"{_holed(ns) if holed else _contiguous(ns)} {_contiguous(nm)} {_contiguous(nh)} * * *"
    if not holed:
        for n in range(1, DAY + 1):
            if DAY // n == target:
                return f"@every {n}s"
    return None


def special_specs():
    """rules of 63, 64 and 65 fires mod 64 at (or, where no product or period
    gives the length, up to 8 x 64 away from) 64, 576 and 2048"""
    out = []
    for target in SPECIAL_LENGTHS:
        for holed in (False, True):
            for k in (0, 1, -1, 2, -2, 3, -3, 4, -4, 5, -5, 6, -6, 7, -7, 8, -8):
                s = special_length_spec(target + 64 * k, holed) if target + 64 * k >= 64 else None
                if s:
                    out.append(s)
                    break
    return out


@functools.lru_cache(maxsize=None)
def layout(target_E, zone="UTC"):
    """The sized set: E == target_E exactly.  Cycles of the DENSE specs, each
    behind a filler of 0..60 fires chosen so that the dense run starts on a
    residue mod 64 that its form has not started on yet; every third cycle 200
    empty rules and 70 one-fire rules; then the special lengths, long runs
    that start exactly on a 2048-boundary behind empty rules, rules that close
    the gap and trailing one-fire fillers."""
    t0 = T0 if zone == "UTC" else LORD_HOWE_T0
    t1 = t0 + DAY

    def count(s):
        return counts_of([s], zone, t0, t1)[0]

    assert count(filler(1)) == 1 and count(EMPTY) == 0
    on_cut = ("*/7 * * * * *", "5/10 * * * * *", f"* {FIB} * * * *", "@every 2s")
    tail = special_specs()
    tail_fires = sum(count(s) for s in tail) + sum(count(s) for s in on_cut) + len(on_cut) * SLICE
    assert target_E > 2 * tail_fires, "target_E too small for the fixed part of the layout"
    specs, pos, cycle = [], 0, 0
    seen = {f: set() for f in FORMS}
    rot = 0
    full = False
    while not full:
        for d in DENSE:
            n = count(d)
            if pos + 60 + n + tail_fires > target_E:
                full = True
                break
            form = spec_form(d, n, zone, t0, t1)
            want = [k for k in range(61) if (pos + k) % 64 not in seen[form]]
            k = want[0] if want else rot % 61
            rot += 7
            specs += [filler(k), d]
            seen[form].add((pos + k) % 64)
            pos += count(filler(k)) + n
        cycle += 1
        if not full and cycle % 3 == 0 and pos + 70 + tail_fires <= target_E:
            specs += [EMPTY] * 200 + [filler(1)] * 70
            pos += 70
    for s in tail:
        specs.append(s)
        pos += count(s)
    for s in on_cut:  # a long run that starts on a slice boundary, empty rules right before it
        need = -pos % SLICE
        specs += fillers(need) + [EMPTY] * 3 + [s]
        pos += need + count(s)
    for s in GAP_MENU:
        n = count(s)
        while n > 0 and pos + n <= target_E:
            specs.append(s)
            pos += n
    assert 0 <= target_E - pos < 1000, (target_E, pos)
    specs += [filler(1)] * (target_E - pos)
    case = make_case(f"layout({target_E}, {zone})", specs, zone, t0, t1)
    assert int(case.off[-1]) == target_E
    return case


def extended(case, k):
    """case with k more trailing one-fire fillers"""
    specs = case.specs + [filler(1)] * k
    return make_case(f"{case.name}+{k}", specs, case.zone, case.t0, case.t1)


def extend_csr(case, eo, et, k):
    """the oracle CSR (eo, et) of `case`, extended to extended(case, k)'s in numpy"""
    one = O.expand_batch(O.sched_array(oracle_parse_all([filler(1)])), case.t0, case.t1, oracle_zone(case.zone))[1]
    assert one.size == 1
    return (np.concatenate([eo, eo[-1] + 1 + np.arange(k, dtype=np.int64)]),
            np.concatenate([et, np.repeat(one, k)]))


# sizes: the position-slice mode starts at E = 2^25 (capacity below 2^31)
E_POSITION = (1 << 25) + 5003
E_EDGE = (1 << 25) - 1
E_MID = 5_000_011


def u_shift(U):
    """cg_kernels.h u_shift: the cost shift of a short window's slices"""
    s = 6
    while (U >> s) >= 16384:
        s += 1
    return s
