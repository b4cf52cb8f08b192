"""The rule sets of tests/mask_cases.py hold what they promise, so that a later
edit of the generators cannot empty tests/test_gpu_masks.py unnoticed.  The
oracle alone satisfies every condition here: they are statements about the
inputs, not measurements of the library."""
import numpy as np
import pytest

import mask_cases as M
import oracle_lib as O
import writer_cases as W
from cronsun_amd import cron, synth

T0, T1 = synth.T0_2026 + 1234, synth.T0_2026 + W.DAY
SEED = 1


def popcount(x, width):
    return bin(int(x) & ((1 << width) - 1)).count("1")


@pytest.fixture(scope="module")
def day():
    specs = M.stratified(360, SEED)
    return specs, np.array(W.counts_of(specs, "UTC", T0, T1), dtype=np.int64)


def test_stratified_radices(day):
    specs, _ = day
    seen = {"S": set(), "M": set(), "H": set()}
    for i, sp in enumerate(specs):
        s = O.parse(sp)[0].spec
        got = popcount(s.second, 60), popcount(s.minute, 60), popcount(s.hour, 24)
        assert got == M.radices(i), (i, sp)
        for k, v in zip("SMH", got):
            seen[k].add(v)
    assert seen["S"] == seen["M"] == set(range(1, 61)) and seen["H"] == set(range(1, 25))
    assert len({M.radices(i) for i in range(360)}) == 120


def test_stratified_day_fields(day):
    specs, _ = day
    star = 1 << 63
    for i, sp in enumerate(specs):
        s = O.parse(sp)[0].spec
        assert (bool(s.dom & star), bool(s.dow & star)) == ((True, True), (False, True), (True, False),
                                                            (False, False))[i % 4], (i, sp)
        assert (sp.split(" ")[4] != "*") == (i % 5 == 0)
        assert not s.month & star or i % 5 != 0


def test_stratified_sparse_caps_the_seconds():
    specs = M.stratified(240, SEED, sparse=True)
    nS = [popcount(O.parse(sp)[0].spec.second, 60) for sp in specs]
    assert set(nS) == {1, 2, 3}
    nM = {popcount(O.parse(sp)[0].spec.minute, 60) for sp in specs}
    assert nM == set(range(1, 61))
    assert M.stratified(240, SEED, sparse=True) == specs and M.stratified(240, SEED + 1, sparse=True) != specs


def test_stratified_fires_and_forms(day):
    specs, cnt = day
    long_runs = [i for i in range(len(specs)) if cnt[i] >= 64]
    assert len(long_runs) >= 300
    forms = [W.spec_form(specs[i], int(cnt[i]), "UTC", T0, T1) for i in long_runs]
    assert forms.count("table") >= 250
    assert 2_000_000 <= int(cnt.sum()) <= 8_000_000


def same_masks(specs):
    for sp in specs:
        o, err = O.parse(sp)
        assert err is None, (sp, err)
        p = cron.Parse(sp)
        assert (p.Second, p.Minute, p.Hour, p.Dom, p.Month, p.Dow) == (
            o.spec.second, o.spec.minute, o.spec.hour, o.spec.dom, o.spec.month, o.spec.dow), sp


def test_both_parsers_agree(day):
    same_masks(day[0])
    same_masks(M.stratified(240, SEED, sparse=True))
    same_masks(M.extremes())


def test_extremes_hold_every_pattern():
    named = M.extremes_named()
    names = [n for n, _ in named]
    assert len(set(names)) == len(names)
    want = []
    for level in ("second", "minute"):
        want += [f"{level}/{p}" for p in (
            "bit0", "top", "0+top", "31+32", "bits32-59", "bits0-31", "all-but-0", "all-but-31", "all-but-32",
            "all-but-59", "even", "odd", "ap-first>=step", "ap-step-not-dividing", "ap-minus-one", "ap-plus-one")]
    want += [f"hour/{p}" for p in ("bit0", "top", "0+top", "all-but-0", "all-but-23", "even", "odd", "ap-first>=step",
                                   "ap-step-not-dividing", "ap-minus-one", "ap-plus-one", "1,2,4,8,16", "0,23")]
    want += [f"day/{p}" for p in ("dom-1,2,4,8,16,31", "dom-31", "dow-Mon,Tue,Thu")]
    for w in want:
        assert f"{w}/star" in names and f"{w}/table" in names, w
    assert {"never/empty-hour", "never/empty-dom", "never/empty-month"} <= set(names)
    # the masks are what their names say
    by = dict(named)
    bit = lambda *v: sum(1 << x for x in v)  # noqa: E731
    full60, m60 = bit(*range(60)), (1 << 60) - 1
    for k, level in enumerate(("second", "minute")):
        mask = lambda name: [O.parse(by[f"{level}/{name}/table"])[0].spec.second,  # noqa: E731
                             O.parse(by[f"{level}/{name}/table"])[0].spec.minute][k] & m60
        assert mask("bit0") == 1 and mask("top") == bit(59) and mask("0+top") == bit(0, 59)
        assert mask("31+32") == bit(31, 32) and mask("bits32-59") == full60 & ~((1 << 32) - 1)
        assert mask("bits0-31") == (1 << 32) - 1
        for h in (0, 31, 32, 59):
            assert mask(f"all-but-{h}") == full60 & ~bit(h)
        assert mask("even") == bit(*range(0, 60, 2)) and mask("odd") == bit(*range(1, 60, 2))
        assert mask("ap-first>=step") == bit(*range(7, 60, 5)) and mask("ap-step-not-dividing") == bit(*range(0, 60, 7))
        for near in ("ap-minus-one", "ap-plus-one"):
            m = mask(near)
            assert not W.is_ap(m) and bin(m ^ bit(*range(3, 60, 4))).count("1") == 1
    hour = lambda name: O.parse(by[f"hour/{name}/star"])[0].spec.hour & 0xFFFFFF  # noqa: E731
    assert hour("top") == bit(23) and hour("0+top") == hour("0,23") == bit(0, 23) and hour("1,2,4,8,16") == bit(1, 2, 4, 8, 16)
    assert hour("all-but-23") == 0x7FFFFF and not W.is_ap(hour("ap-minus-one")) and not W.is_ap(hour("ap-plus-one"))
    # the other levels of a '/table' variant are no progressions
    for n, sp in named:
        if n.endswith("/table") and not n.startswith("day/"):
            s = O.parse(sp)[0].spec
            others = [m for lv, m in zip(M.LEVELS, (s.second & m60, s.minute & m60, s.hour & 0xFFFFFF)) if lv != n.split("/")[0]]
            assert not any(W.is_ap(m) for m in others), n


def test_extremes_forms():
    specs = M.extremes()
    cnt = W.counts_of(specs, "UTC", T0, T1)
    forms = {W.spec_form(sp, n, "UTC", T0, T1) for sp, n in zip(specs, cnt)}
    assert forms >= {"linear", "affine", "table", "tiny", "empty"}
    by = dict(M.extremes_named())
    # the never-firing rules never fire: no fire in 40 days either
    never = [by[n] for n in ("never/empty-hour", "never/empty-dom", "never/empty-month")]
    assert W.counts_of(never, "UTC", T0, T0 + 40 * W.DAY) == [0, 0, 0]
    assert set(never) <= set(M.day_extremes()) and len(M.day_extremes()) == 9


def test_long_horizon_day_sets_are_tables():
    """Over 40 days from a midnight - 77 s most day lists are no progression
    (three rules in four have one), and the sparse day extremes keep their day
    fields with three second bits."""
    t0, t1 = synth.T0_2026 - 77, synth.T0_2026 + 40 * W.DAY
    days = W.window_days("UTC", t0, t1)
    assert len(days) == 42 and days[0].month != days[-1].month  # 4 Jan 23:58:44 .. 14 Feb 00:00:00
    specs = M.stratified(240, SEED, sparse=True)
    tables = sum(not W.is_ap(W.day_mask(O.parse(sp)[0], days)) for sp in specs)
    assert tables >= 150
    dense, sparse = M.day_extremes(), M.day_extremes(sparse=True)
    same_masks(sparse)
    changed = 0
    for a, b in zip(dense, sparse):
        assert a.split(" ")[1:] == b.split(" ")[1:]
        if a != b:
            changed += 1
            assert a.startswith("* * * ") and popcount(O.parse(b)[0].spec.second, 60) == 3
    assert changed == 3
    for sp in sparse[:6]:
        assert not W.is_ap(W.day_mask(O.parse(sp)[0], days)) or " 31 " in sp


def test_junk_bits():
    cols = M.soa_columns(M.stratified(360, SEED) + M.extremes())
    junk = M.junk_bits(cols, 7)
    looked_at = {"second": (1 << 60) - 1, "minute": (1 << 60) - 1, "hour": (1 << 24) - 1, "dom": 0xFFFFFFFE,
                 "month": 0x1FFE, "dow": 0x7F}
    for name, a, b in zip(M.COLUMNS, cols, junk):
        keep = np.uint64(looked_at[name] | 1 << 63)
        assert looked_at[name] & M.junk_mask(name) == 0 and looked_at[name] | M.junk_mask(name) == (1 << 63) - 1
        assert np.array_equal(a & keep, b & keep) and np.array_equal(a, b & ~np.uint64(M.junk_mask(name)))
        added = np.bitwise_or.reduce(a ^ b)
        assert int(added) == M.junk_mask(name), name  # every junk bit is set in some rule
