"""The LDS-sliced scatter-add (csrc/hash_bwd_lds.hip: ngp_hash_bwd_f32_sliced, ngp_hash_bwd_sliced_prep / _main / _main_f16) against
the term-by-term float64 reference of tests/hash_scatter_reference.py, element by element, at the bound that module derives from
the kernel's arithmetic: the products are summed in float64 and rounded once, so a single owner's element is fl32(sum) up to rounding
ties, not "within 2e-5".

The inputs (hash_scatter_reference: one_cell, pieces, mixed) are the smallest that run the owner loop's (bwd_task) rarely used
parts -- more than 64 non-empty pieces per super-chunk, a queue that fills by 64 and drains at exactly 128, the ring's wrap-around,
run pre-sums over whole rows and across row / batch / super-chunk boundaries, replicas with an empty sample range -- on the default
training table (C2), the C3 table in its default and concentrated plans, a table whose hashed levels take the real modulo
(KIND_GENERIC) and one whose finest levels have res >= 2^13 (where the two-multiply hashed form must not be taken).

Every launch is compared on the device at the elements the reference lists; every other element of the table must keep its fill
bits.  Per table and variant the worst error / bound is printed by level class (single-owner non-merge, merge, replicated).  On
the single-owner non-merge levels onto zeros every element that is not within k 2^-52 S of a rounding boundary must equal
fl32(sum) (half2: fl16(fl32(sum))) bit for bit, and at least 99 % of all of them must."""
import ctypes

import numpy as np
import pytest
import torch

import hash_scatter_reference as hs

pytestmark = pytest.mark.gpu
DEV = "cuda"
f16, f32, f64 = np.float16, np.float32, np.float64
_cache = {}

# table name -> (hs.TABLES key, plan bits by name)
PLANS = {"C2": ("C2", ""), "C3": ("C3", ""), "C3_concentrated": ("C3", "concentrated"), "real_modulo": ("real_modulo", ""), "fine": ("fine", ""),
         "C2_deterministic": ("C2", "deterministic")}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _table(name):
    """Level table (with its plan bits), its plan and the cached inputs of the underlying table."""
    if name not in _cache:
        from ngp_hip import lib, ops
        key, mode = PLANS[name]
        lv = ops.make_levels(*hs.TABLES[key])
        if mode:
            lv = lv.with_plan({"concentrated": lib.BWD_PLAN_CONCENTRATED, "deterministic": lib.BWD_PLAN_DETERMINISTIC}[mode])
        n_tasks, nrep, merge_mask = hs.sliced_plan(lv)
        _cache[name] = dict(lv=lv, n_tasks=n_tasks, nrep=nrep, merge_mask=merge_mask, size=lv.total_entries * 2, key=key)
        print("%s: plan of %d tasks, nrep %s, merge mask 0x%x" % (name, n_tasks, [int(v) for v in nrep], merge_mask))
    return _cache[name]


def _input(key, what, make):
    """Inputs and references are computed once per underlying table and shared, unchanged, by the tests that need them."""
    k = ("input", key, what)
    if k not in _cache:
        _cache[k] = make()
    return _cache[k]


def _refused(t, hip_lib):
    """The fine table: if the plan refuses it, so must the entry point, and the case ends there."""
    if t["n_tasks"] != -2:
        assert t["n_tasks"] > 0
        return False
    from ngp_hip import ops
    with pytest.raises(RuntimeError, match="code -2"):
        ops.hash_bwd_f32_sliced(torch.rand(100, 3, device=DEV), torch.zeros(100, 32, device=DEV), t["lv"], torch.zeros(t["size"], device=DEV))
    return True


# ------------------------------------------------------------------------------------------------ launches
def _pair_major(g):
    """[n, 32] rows as the fused path's eight pair-major planes [8][n][4] (plane p = levels p and 15 - p)."""
    n = g.shape[0]
    g = g.reshape(n, 16, 2)
    pm = torch.zeros(8, n, 4, device=g.device)
    for l in range(16):
        pm[l if l < 8 else 15 - l, :, (0 if l < 8 else 2):(2 if l < 8 else 4)] = g[:, l]
    return pm.contiguous()


def _launch(t, x, g, fill=0.0, form="f32", live=None, n_dev=None):
    """One launch onto a table filled with `fill`; returns the table.  form: f32 (ngp_hash_bwd_f32_sliced), pairs (prepass + main on
    the pair-major layout), half (prepass + main_f16)."""
    from ngp_hip import lib as L, ops
    from ngp_hip.ops import _ptr, _stream
    lv, n = t["lv"], g.shape[0]
    lib = L.load()
    if form == "half":
        table = torch.full((lv.total_entries, 2), fill, device=DEV, dtype=torch.float16)
        ops.hash_bwd_f16_sliced(x, g, lv, table, live_idx=live, n_dev=n_dev)
    elif form == "pairs":
        table = torch.full((t["size"],), fill, device=DEV)
        ws = ops.sliced_workspace(lv, n, x.device)
        L.check(lib.ngp_hash_bwd_sliced_prep(_ptr(x), ctypes.byref(lv), n, _ptr(n_dev), _ptr(live), 0, 0.0, 1.0, _ptr(ws), ws.numel(),
                                             _stream()), "ngp_hash_bwd_sliced_prep")
        pm = _pair_major(g)
        L.check(lib.ngp_hash_bwd_sliced_main(_ptr(pm), ctypes.byref(lv), n, _ptr(n_dev), 1, _ptr(table), _ptr(None), _ptr(ws), ws.numel(),
                                             _stream()), "ngp_hash_bwd_sliced_main")
        torch.cuda.synchronize()                                    # (pm stays alive until the launch has read it)
    else:
        table = torch.full((t["size"],), fill, device=DEV)
        ops.hash_bwd_f32_sliced(x, g, lv, table, live_idx=live, n_dev=n_dev)
    torch.cuda.synchronize()
    return table


def _launch_normalised(t, x, g, lo, hi):
    """ngp_hash_bwd_f32_sliced itself with its fused normalisation switched on."""
    from ngp_hip import lib as L, ops
    from ngp_hip.ops import _ptr, _stream
    lv, n = t["lv"], g.shape[0]
    table = torch.zeros(t["size"], device=DEV)
    ws = ops.sliced_workspace(lv, n, x.device)
    L.check(L.load().ngp_hash_bwd_f32_sliced(_ptr(x), _ptr(g), ctypes.byref(lv), n, _ptr(None), _ptr(None), 1, lo, hi, 0, _ptr(table), _ptr(None),
                                             _ptr(ws), ws.numel(), _stream()), "ngp_hash_bwd_f32_sliced")
    torch.cuda.synchronize()
    return table


# ------------------------------------------------------------------------------------------------ the comparison
class Tally:
    """Worst error / bound per level class and the bit-exact count of one (table, variant), over all its launches."""

    def __init__(self, what):
        self.what, self.worst, self.exact, self.single, self.elements = what, [0.0, 0.0, 0.0], 0, 0, 0

    def close(self, expect_exact=True):
        print("%s: %d elements; worst error / bound: %s; bit-exact %d of %d single-owner non-merge elements onto zeros"
              % (self.what, self.elements, ", ".join("%s %.3f" % (hs.CLASS_NAMES[c], self.worst[c]) for c in range(3)), self.exact, self.single))
        if expect_exact:
            assert self.single > 0 and self.exact >= 0.99 * self.single, (self.what, self.exact, self.single)


def _check(got, sc, t, fill, half, tally, what):
    """got: the whole table after a launch onto `fill` (device).  No element is left out: those the reference lists hold the bound,
    all others keep fill's bits."""
    assert sc.entries.size > 0
    flat = got.reshape(-1)
    assert flat.numel() == t["size"]
    e = _dev(sc.entries)
    keep = torch.ones(flat.numel(), dtype=torch.bool, device=DEV)
    keep[e] = False
    if half:
        fill_bits = int(np.full(1, fill, dtype=f16).view(np.int16)[0])
        assert bool((flat.view(torch.int16)[keep] == fill_bits).all()), "%s: an element without a term changed" % what
    else:
        fill_bits = int(np.full(1, fill, dtype=f32).view(np.int32)[0])
        assert bool((flat.view(torch.int32)[keep] == fill_bits).all()), "%s: an element without a term changed" % what
    vals = flat[e]
    err = (vals.double() - fill - _dev(sc.sum)).abs()
    ratio = err / _dev(hs.bound(sc, t["lv"], t["nrep"], t["merge_mask"], fill, half))
    cls = hs.level_class(hs.level_of(sc.entries, t["lv"]), t["nrep"], t["merge_mask"])
    cls_d = _dev(cls)
    tally.elements += int(sc.entries.size)
    for c in range(3):
        if np.any(cls == c):
            tally.worst[c] = max(tally.worst[c], float(ratio[cls_d == c].max()))
    if fill == 0.0 and np.any(cls == hs.SINGLE):
        same = vals.float() == _dev(hs.rounded(sc, half))           # (neither side is NaN; a zero sum is +0 on both)
        single = cls_d == hs.SINGLE
        must = single & ~_dev(hs.near_tie(sc, half))
        assert bool(same[must].all()), "%s: a single-owner element away from any rounding boundary is not the rounded sum" % what
        tally.exact += int((same & single).sum())
        tally.single += int(single.sum())
    worst = float(ratio.max())
    assert worst <= 1.0, "%s onto %g: error / bound = %.4g" % (what, fill, worst)


# ------------------------------------------------------------------------------------------------ one cell
def _one_cell(key, half=False):
    def make():
        from ngp_hip import ops
        lv = ops.make_levels(*hs.TABLES[key])
        x, g = hs.one_cell(lv, half=half)                           # asserts the structure
        pre = hs.prefix_scatters(x, g, lv, hs.PREFIXES, half)
        if half:
            assert not any(np.any(sc.k_sub) for sc in pre.values()), "a half2 term of the one-cell set is an f16 subnormal"
        return _dev(x), _dev(g), pre
    return _input(key, "one_cell_half" if half else "one_cell", make)


def _run_prefixes(t, name, fill=0.0, form="f32", twice=False):
    half = form == "half"
    x, g, pre = _one_cell(t["key"], half)
    tally = Tally("one cell, %s, %s onto %g" % (name, form, fill))
    for n in hs.PREFIXES:
        got = _launch(t, x[:n].contiguous(), g[:n].contiguous(), fill, form)
        _check(got, pre[n], t, fill, half, tally, "%s n=%d" % (tally.what, n))
        if twice:
            again = _launch(t, x[:n].contiguous(), g[:n].contiguous(), fill, form)
            assert torch.equal(got.view(torch.int32), again.view(torch.int32)), "%s n=%d: two launches differ" % (tally.what, n)
    tally.close(expect_exact=fill == 0.0)


@pytest.mark.parametrize("name", ["C2", "C3", "C3_concentrated", "real_modulo", "fine"])
def test_one_cell_prefixes(hip_lib, name):
    """Natural layout onto zeros, every prefix of the one-cell set, on every table and plan."""
    t = _table(name)
    if _refused(t, hip_lib):
        return
    _run_prefixes(t, name)


@pytest.mark.parametrize("variant", ["ones", "pairs", "deterministic", "half"])
def test_one_cell_variants(hip_lib, variant):
    """C2: accumulate-into (a table of ones), the pair-major layout through prepass + main, the deterministic plan (two launches
    bit-identical on the whole table), the half2 form (|g| in [1, 2): no f16-subnormal term)."""
    if variant == "deterministic":
        t = _table("C2_deterministic")
        assert np.all(t["nrep"] == 1)
        _run_prefixes(t, "C2_deterministic", twice=True)
    else:
        _run_prefixes(_table("C2"), "C2", fill=1.0 if variant == "ones" else 0.0, form={"ones": "f32"}.get(variant, variant))


# ------------------------------------------------------------------------------------------------ pieces
@pytest.mark.parametrize("by", [1, 8])
@pytest.mark.parametrize("name", ["C2", "C3", "C3_concentrated", "real_modulo", "fine"])
def test_pieces(hip_lib, name, by):
    """Two cells alternating by sample parity and by 8-sample piece: natural layout onto zeros."""
    t = _table(name)
    if _refused(t, hip_lib):
        return

    def make():
        x, g = hs.pieces(t["lv"], by)                               # asserts the structure
        return _dev(x), _dev(g), hs.scatter(x, g, t["lv"])
    x, g, sc = _input(t["key"], "pieces_%d" % by, make)
    tally = Tally("pieces by %d, %s" % (by, name))
    _check(_launch(t, x, g), sc, t, 0.0, False, tally, tally.what)
    tally.close()


# ------------------------------------------------------------------------------------------------ mixed
def _mixed(what):
    def make():
        from ngp_hip import ops
        lv = ops.make_levels(*hs.TABLES["C2"])
        x, g, perm, m = hs.mixed()
        if what == "live":
            return _dev(x), _dev(g), hs.scatter(x, g, lv, live_idx=perm, count=m), _dev(perm), torch.tensor([m], device=DEV, dtype=torch.int32)
        if what == "normalised":
            raw, x01 = hs.normalised(x, -0.5, 0.5)
            return _dev(raw), _dev(g), hs.scatter(x01, g, lv)
        return _dev(x), _dev(g), hs.scatter(x, g, lv, half=what == "half")
    return _input("C2", "mixed_" + what, make)


@pytest.mark.parametrize("variant", ["zeros", "ones", "pairs", "deterministic", "half", "live", "normalised"])
def test_mixed(hip_lib, variant):
    """C2, rays + uniform points + the box's corners + zero rows: every variant of the one-cell test, then through a permuted live
    list with a device count below n_max, and with the fused normalisation lo, hi = -0.5, 0.5."""
    t = _table("C2_deterministic" if variant == "deterministic" else "C2")
    tally = Tally("mixed, C2, %s" % variant)
    if variant == "live":
        x, g, sc, perm, cnt = _mixed("live")
        got = _launch(t, x, g, live=perm, n_dev=cnt)
        _check(got, sc, t, 0.0, False, tally, tally.what)
    elif variant == "normalised":
        x, g, sc = _mixed("normalised")
        _check(_launch_normalised(t, x, g, -0.5, 0.5), sc, t, 0.0, False, tally, tally.what)
    else:
        half = variant == "half"
        x, g, sc = _mixed("half" if half else "plain")
        fill = 1.0 if variant == "ones" else 0.0
        form = variant if variant in ("pairs", "half") else "f32"
        got = _launch(t, x, g, fill, form)
        _check(got, sc, t, fill, half, tally, tally.what)
        if variant == "deterministic":
            assert np.all(t["nrep"] == 1)
            again = _launch(t, x, g, fill, form)
            assert torch.equal(got.view(torch.int32), again.view(torch.int32)), "two launches of the deterministic plan differ"
    tally.close(expect_exact=variant != "ones")
