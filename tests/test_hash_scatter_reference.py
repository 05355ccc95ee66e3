"""tests/hash_scatter_reference.py against the oracle, and the structure its input builders promise -- no GPU.

The oracle (ora_hash_bwd_f32 / ora_hash_bwd_f16) adds the same float32 (half2: f16-rounded) products in float64 in sample order and
rounds once to float32, so it must have the reference's support and lie within oracle_bound of its sums: one float32 rounding of
the sum plus the float64 accumulation error of both sides, k 2^-52 S, computed per element from S.  (A serial float32 sum would be
allowed k 2^-24 S; the oracle is held to the tighter figure that its own arithmetic gives.)"""
import math

import numpy as np
import pytest

import hash_scatter_reference as hs

f16, f32, f64 = np.float16, np.float32, np.float64
_cache = {}


def _levels(table):
    from ngp_hip import ops
    return ops.make_levels(*hs.TABLES[table])


def _inputs(table):
    """name -> (x, g, live_idx, count) for one table; every builder asserts its structure while it runs."""
    if table not in _cache:
        lv = _levels(table)
        sets = {"one_cell": hs.one_cell(lv) + (None, None), "one_cell_half": hs.one_cell(lv, half=True) + (None, None),
                "pieces_1": hs.pieces(lv, 1) + (None, None), "pieces_8": hs.pieces(lv, 8) + (None, None)}
        x, g, perm, m = hs.mixed()
        sets["mixed"] = (x, g, None, None)
        sets["mixed_live"] = (x, g, perm, m)
        sets["mixed_normalised"] = (hs.normalised(x, -0.5, 0.5)[1], g, None, None)
        _cache[table] = (lv, sets)
    return _cache[table]


SETS = ("one_cell", "one_cell_half", "pieces_1", "pieces_8", "mixed", "mixed_live", "mixed_normalised")


def _against_oracle(want, sc, size, what):
    want = np.asarray(want, dtype=f64).reshape(-1)
    assert want.size == size
    touched = np.zeros(size, dtype=bool)
    touched[sc.entries] = True
    assert not np.any(want[~touched]), "%s: the oracle is nonzero where the reference has no term" % what
    err = np.abs(want[sc.entries] - sc.sum)
    ratio = float(np.max(err / hs.oracle_bound(sc)))
    print("%s: %d elements, worst |oracle - ref| / bound = %.3f" % (what, sc.entries.size, ratio))
    assert ratio <= 1.0, (what, ratio)
    # same support: an element with terms is zero in the oracle only where its sum rounds to zero
    assert np.all((want[sc.entries] != 0) == (sc.sum.astype(f32) != 0)), "%s: support differs" % what


@pytest.mark.parametrize("name", SETS)
@pytest.mark.parametrize("table", list(hs.TABLES))
def test_reference_matches_the_oracle(oracle, table, name):
    lv, sets = _inputs(table)
    x, g, live, count = sets[name]
    n = g.shape[0] if count is None else count
    xs = x[:n] if live is None else x[live[:n]]
    size = lv.total_entries * lv.n_features
    sc = hs.scatter(x, g, lv, live_idx=live, count=count)
    assert sc.entries.size > 0 and np.all(sc.S > 0) and np.all(sc.k > 0) and np.all(np.abs(sc.sum) <= sc.S)
    _against_oracle(oracle.hash_bwd_f32(xs, g[:n], lv), sc, size, "f32 %s %s" % (table, name))
    sch = hs.scatter(x, g, lv, half=True, live_idx=live, count=count)
    _against_oracle(oracle.hash_bwd_f16(xs, g[:n].reshape(n, lv.n_levels, lv.n_features).astype(f16), lv), sch, size,
                    "half2 %s %s" % (table, name))
    if name == "one_cell_half":
        assert not np.any(sch.k_sub), "a half2 term of the one-cell set is an f16 subnormal"
    if name in ("one_cell", "pieces_1", "pieces_8", "mixed"):
        assert float(np.min(np.abs(g[g != 0]))) >= 2.0**-20 and float(np.max(np.abs(g))) <= 4.0


@pytest.mark.parametrize("table", list(hs.TABLES))
def test_prefix_sums_are_the_scatter_of_the_prefix(table):
    """The one-cell set's cumulative reference equals the scatter of each prefix, and the serial float64 sums equal math.fsum of
    the terms to within the (k - 1) 2^-53 S that the bound carries for them."""
    lv, sets = _inputs(table)
    for name, half in (("one_cell", False), ("one_cell_half", True)):
        x, g = sets[name][:2]
        pre = hs.prefix_scatters(x, g, lv, hs.PREFIXES, half)
        for n in (1, 65, 129, 4097, hs.N_ONE_CELL):
            sc = hs.scatter(x[:n], g[:n], lv, half)
            assert np.array_equal(sc.entries, pre[n].entries) and np.array_equal(sc.k, pre[n].k) and np.array_equal(sc.k_sub, pre[n].k_sub)
            assert np.all(np.abs(sc.sum - pre[n].sum) <= sc.k * 2.0**-52 * sc.S) and np.allclose(sc.S, pre[n].S, rtol=1e-12, atol=0)
        flat, p = hs.terms(x, g, lv, half)
        flat, p = flat.reshape(-1), p.reshape(-1).astype(f64)
        full = pre[hs.N_ONE_CELL]
        for j in range(0, full.entries.size, 7):
            exact = math.fsum(p[flat == full.entries[j]])
            assert abs(exact - full.sum[j]) <= (full.k[j] - 1) * 2.0**-53 * full.S[j]
        assert 2 * 8 * lv.n_levels >= full.entries.size >= 2 * 8 * lv.begin_fast_hash_level        # dense corners are distinct
        assert int(full.k.max()) <= 8 * (hs.N_ONE_CELL - len(hs.ONE_CELL_ZERO_ROWS))
        assert int(full.k.min()) >= hs.N_ONE_CELL - len(hs.ONE_CELL_ZERO_ROWS)


@pytest.mark.parametrize("table", list(hs.TABLES))
def test_few_sums_lie_on_a_rounding_boundary(table):
    """The GPU test demands that at least 99 % of the single-owner non-merge elements equal fl32(sum) (half2: fl16(fl32(sum))) bit
    for bit; the rest may only be sums within k 2^-52 S of a rounding boundary.  Fewer than 1 % of the reference's elements are."""
    lv, sets = _inputs(table)
    n_tasks, nrep, merge_mask = hs.sliced_plan(lv)
    if n_tasks == -2:                                               # the sliced formulation refuses this table: nothing to round
        return
    assert n_tasks > 0
    # the (input set, form) pairs the GPU test launches; the one-cell sets count over all their prefixes, as the GPU test does
    for name, half in (("one_cell", False), ("one_cell_half", True), ("pieces_1", False), ("pieces_8", False), ("mixed", False),
                       ("mixed", True), ("mixed_live", False), ("mixed_normalised", False)):
        x, g, live, count = sets[name]
        scs = list(hs.prefix_scatters(x, g, lv, hs.PREFIXES, half).values()) if name.startswith("one_cell") else [hs.scatter(x, g, lv, half, live, count)]
        ties = total = 0
        for sc in scs:
            single = hs.level_class(hs.level_of(sc.entries, lv), nrep, merge_mask) == hs.SINGLE
            ties += int(hs.near_tie(sc, half)[single].sum())
            total += int(single.sum())
        assert total > 0
        print("%s %s half=%d: %d single-owner elements, %.4f %% near a rounding boundary" % (table, name, half, total, 100.0 * ties / total))
        assert ties < 0.01 * total


def test_builders_are_reproducible_and_the_bound_is_finite():
    lv = _levels("C2")
    x, g = hs.one_cell(lv)
    x2, g2 = hs.one_cell(lv)
    assert np.array_equal(x, x2) and np.array_equal(g, g2)
    assert not np.any(g[list(hs.ONE_CELL_ZERO_ROWS)])
    n_tasks, nrep, merge_mask = hs.sliced_plan(lv)
    sc = hs.scatter(x[:300], g[:300], lv)
    for fill in (0.0, 1.0):
        b = hs.bound(sc, lv, nrep, merge_mask, fill)
        assert np.all(np.isfinite(b)) and np.all(b >= 2.0**-24 * np.abs(sc.sum)) and np.all(b <= 2.0**-17 * (fill + sc.S) + 2.0**-149)
