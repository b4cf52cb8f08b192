"""The constructed rule sets of tests/writer_cases.py hold the cases they
promise.  The oracle alone satisfies every condition here; they keep
tests/test_gpu_writer.py from passing because a case went missing."""
import numpy as np
import pytest

import oracle_lib as O
import writer_cases as W
from common import oracle_parse_all, oracle_zone

F = {f: i for i, f in enumerate(W.FORMS)}


def oracle_offsets(case):
    arr = O.sched_array(oracle_parse_all(case.specs))
    return O.expand_batch(arr, case.t0, case.t1, oracle_zone(case.zone), threads=8, with_times=False)[0]


def test_is_ap():
    def mask(vals):
        return sum(1 << v for v in vals)
    assert W.is_ap(0) and W.is_ap(mask([7])) and W.is_ap(mask([3, 50]))
    assert W.is_ap(mask(range(0, 60, 7))) and W.is_ap(mask(range(5, 60, 10))) and W.is_ap(mask(range(60)))
    assert not W.is_ap(mask([1, 2, 3, 5, 8])) and not W.is_ap(mask([0, 1, 3])) and not W.is_ap(mask([0, 2, 4, 7]))


@pytest.mark.parametrize("spec,form", [
    ("*/10 * * * * *", "linear"), ("5/10 * * * * *", "linear"), ("0 */5 * * * *", "linear"),
    ("*/7 * * * * *", "affine"), ("0-29 * * * * *", "affine"), ("*/10 0-58 * * * *", "affine"),
    ("* * 0-22 * * *", "affine"), ("*/2 * 1 * * *", "affine"),
    ("1,2,3,5,8,13,21,34,55 * * * * *", "table"), ("* 1,2,3,5,8,13,21,34,55 * * * *", "table"),
    ("@every 7s", "every")])
def test_forms_of_the_documented_examples(spec, form):
    t0, t1 = W.T0, W.T0 + W.DAY
    n = W.counts_of([spec], "UTC", t0, t1)[0]
    assert n >= 64 and W.spec_form(spec, n, "UTC", t0, t1) == form
    days20 = (W.T0, W.T0 + 20 * W.DAY)
    assert W.spec_form("0 0 * * * 1-5", 336, "UTC", *days20) == "table"
    assert W.spec_form("0 0 * * * Mon", 72, "UTC", *days20) == "affine"
    assert W.spec_form("@every 7s", 5, "UTC", t0, t0 + 35) == "tiny"


def test_sweep_holds_every_target():
    gens = {g: i for i, g in enumerate(W.SWEEP_GENS)}
    for L in W.SWEEP_L:
        case = W.sweep(L)
        assert np.array_equal(case.off, oracle_offsets(case))
        E, R = int(case.off[-1]), len(case.specs)
        assert E + R < 1 << 20 and W.u_shift(E + R) == 6
        lg = case.ledger
        seen, forms = set(), set()
        for i, s in enumerate(case.specs):
            if s in gens:
                seen.add((s, int(lg.residue[i])))
                if lg.count[i] >= 64:
                    forms.add((int(lg.form[i]), int(lg.residue[i])))
        assert seen == {(g, r) for g in W.SWEEP_GENS for r in W.RESIDUES}, L
        # the unconfined generators and, from L = 127 on, the confined ones are long
        want = [F["linear"], F["every"]] + ([F["affine"], F["table"]] if L >= 127 else [])
        assert forms >= {(f, r) for f in want for r in W.RESIDUES}, L
        every_second = [i for i, s in enumerate(case.specs) if s == "* * 1 * * *"]
        assert all(lg.count[i] == L + 1 for i in every_second)


@pytest.mark.parametrize("start", W.RADIX_STARTS, ids=["midnight", "7:13:37"])
def test_radices_hold_every_size_and_form(start):
    sizes, forms = {}, {}
    for fam in W.RADIX_FAMILIES:
        case, tags = W.radix_case(fam, start)
        assert case.t0 == start and int(case.off[-1]) <= 10_500_000
        assert (case.ledger.count >= 64).all()
        assert len(tags) == len(case.specs)
        if fam == "day":
            assert all(t[0] == "day" for t in tags)
        for (level, cons, n), f in zip(tags, case.ledger.form):
            sizes.setdefault((level, cons), set()).add(n)
            forms[(level, int(f))] = forms.get((level, int(f)), 0) + 1
    for level, radix in (("second", 60), ("minute", 60), ("hour", 24)):
        assert sizes[(level, "contiguous")] == set(range(1, radix + 1))
        assert sizes[(level, "stepped")] == set(range(1, radix + 1))
        assert sizes[(level, "stepped_high")] == set(range(1, radix + 1))
        assert sizes[(level, "holed")] == set(range(4, radix))
        for f in ("linear", "affine", "table"):
            assert forms.get((level, F[f]), 0) >= 20, (level, f)
    # one time of day per matching day cannot reach 64 fires in 20 days, and
    # with more the days must be consecutive: the day level has no linear form
    assert {c for (lv, c) in sizes if lv == "day"} == set(W.DAY_FIELDS)
    for f in ("affine", "table"):
        assert forms.get(("day", F[f]), 0) >= 20, f


def slice_facts(case):
    """(most runs touched by one 2048-event slice, widest spread of run indices
    feeding one 64-event block), empty runs counted"""
    off, E = case.off, int(case.off[-1])
    out = []
    for width in (W.SLICE, 64):
        lo = np.arange(0, E, width)
        hi = np.minimum(lo + width, E) - 1
        first = np.searchsorted(off, lo, side="right") - 1  # the run holding the first event
        last = np.searchsorted(off, hi, side="right") - 1   # ... and the last
        out.append(int((last - first + 1).max()))
    return tuple(out)


def test_layout_at_position_size():
    case = W.layout(W.E_POSITION)
    off = oracle_offsets(case)
    assert np.array_equal(case.off, off)
    E = int(off[-1])
    assert E == W.E_POSITION and E >= 1 << 25 and E % 64 != 0
    lg = case.ledger
    for f in W.LONG_FORMS:
        rows = (lg.form == F[f]) & (lg.count >= 640)
        assert set(lg.residue[rows].tolist()) == set(range(64)), f
        assert (lg.cut_inside & (lg.form == F[f])).any(), f
    at = np.nonzero(lg.cut_at_start[1:] & (lg.count[:-1] == 0))[0] + 1
    assert at.size and {int(lg.form[i]) for i in at} >= {F[f] for f in W.LONG_FORMS}
    runs_per_slice, spread_per_block = slice_facts(case)
    assert runs_per_slice > 128
    assert spread_per_block > 64
    # the special lengths: 63, 0 and 1 mod 64 near 64, 576 and 2048, with and without a table
    for base in (64, 576, 2048):
        for r in (63, 0, 1):
            near = (lg.count % 64 == r) & (np.abs(lg.count - base) <= 8 * 64 + 1) & (lg.count >= 63)
            assert (near & (lg.form == F["table"])).any() or base == 64, (base, r)
            assert (near & (lg.form != F["table"])).any(), (base, r)


def test_layout_at_the_edge_sizes():
    base = W.layout(W.E_EDGE)
    assert int(base.off[-1]) == (1 << 25) - 1
    small = W.sweep(64)  # the numpy extension of a CSR, against the oracle itself
    arr = O.sched_array(oracle_parse_all(small.specs))
    eo, et = O.expand_batch(arr, small.t0, small.t1, oracle_zone("UTC"))
    for k in (0, 1, 2):
        case = W.extended(base, k)
        assert case.specs[:len(base.specs)] == base.specs and int(case.off[-1]) == (1 << 25) - 1 + k
        assert set(case.specs[len(base.specs):]) <= {W.filler(1)}
        more = W.extended(small, k)
        arr = O.sched_array(oracle_parse_all(more.specs))
        want = O.expand_batch(arr, more.t0, more.t1, oracle_zone("UTC"))
        got = W.extend_csr(small, eo, et, k)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.array_equal(W.extended(base, 2).off, oracle_offsets(W.extended(base, 2)))


@pytest.mark.parametrize("zone", ["UTC", W.LORD_HOWE])
def test_layout_at_the_mid_size(zone):
    case = W.layout(W.E_MID, zone)
    assert np.array_equal(case.off, oracle_offsets(case))
    E = int(case.off[-1])
    assert 1 << 22 <= E < 1 << 23 and W.u_shift(E + len(case.specs)) >= 8
    for f in W.LONG_FORMS:
        assert ((case.ledger.form == F[f]) & case.ledger.cut_inside).any(), f
    if zone != "UTC":  # the window holds the zone's transition
        z = oracle_zone(zone)
        assert z.lookup(case.t0)[0] != z.lookup(case.t1)[0]
