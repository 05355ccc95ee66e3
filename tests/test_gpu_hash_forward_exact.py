"""Every form of the forward hash gather (csrc/hash_grid.hip) against the serial numpy restatement tests/hash_forward_reference.py.

The bar, everywhere: BIT EQUALITY with `forward32` on every element of every row in range; where the reference gives NaN the kernel
gives NaN (a NaN's sign and payload are not part of the contract), and the other elements of such a row are bit-equal.  Every output
buffer is pre-filled with -7 and has 64 spare rows behind it; every row outside the encoded set -- rows >= the device-side count, rows
not in the list, the spare rows, rows [n_dev, n_max) of every pair-major plane -- must keep the fill's bits.  No element is excluded
and there is no tolerance: the comparison is of the whole buffer against the whole expected buffer.

Inputs are the named cases of the reference module (positions uniform in the unit cube behind 17 fixed edge rows: box corners, faces,
a point an ulp inside a cell face of the finest level, points outside the box up to +-1e30, a NaN and a +inf coordinate; signed normal
tables).  The reference of a (table, kind) is computed once over the longest input and sliced.

Which kernel a launch takes (hash_grid.hip's entry points): 16 levels x 2 features with n_max >= 4096 or the pair-major layout -> the
XCD-partitioned kernel, a persistent grid of min(ceil(n_max / 128), 768) tiles, so a lane takes a second trip above 98 304 rows and a
third above 196 608; everything else -> the generic kernel, one lane per (row, level), grid-stride above 4096 * 256 lanes.  The loop
variants NGP_EXPERIMENT selects (one tile, three tiles, the round-1 loop that tables of 4 GB and more get, alone and with one tile) run
in a child process."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import hash_forward_reference as ref
from conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda"
SPARE = 64
LAYOUTS = [0, 1]
LAYOUT_IDS = ["natural", "pair-major"]
SIZES_XCD = (1, 2, 127, 128, 129, 4095, 4096, 4097, ref.N_TRIPS2, ref.N_TRIPS3)
_dev_cache = {}
_child_died = []


def _lib():
    from ngp_hip import ops
    return ops._lib()


def _levels(*shape):
    from ngp_hip import ops
    return ops.make_levels(*shape)


def _case(name):
    """The case, its reference, and its inputs on the device (once)."""
    c = ref.case(name, _levels)
    if name not in _dev_cache:
        t = np.array(c["table"])                                             # (the cached arrays are read-only: upload a copy)
        table = torch.from_numpy(t.view(np.int16)).to(DEV).view(torch.bfloat16) if c["kind"] == "bf16" else torch.from_numpy(t).to(DEV)
        _dev_cache[name] = (torch.from_numpy(np.array(c["x"])).to(DEV), table)
    want = ref.reference(c)
    return c, want.astype(np.float32) if c["kind"] == "f16" else want, _dev_cache[name]


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _stream():
    from ngp_hip import ops
    return ops._stream()


def _buffer(n_max, width, dtype=torch.float32):
    return torch.full(((n_max + SPARE) * width,), -7.0, device=DEV, dtype=dtype)


def _expected(want, rows, n_max, pairs):
    """The whole expected buffer: `want`'s rows `rows` (a slice or an index array) in a buffer of n_max rows, the layout applied,
    the spare rows behind; everything else the fill."""
    width = want.shape[1]
    e = np.full((n_max, width), ref.FILL, dtype=want.dtype)
    e[rows] = want[:n_max][rows]
    if pairs:
        e = ref.to_pair_major(e, n_max)
    return np.concatenate([e.reshape(-1), np.full(SPARE * width, ref.FILL, dtype=want.dtype)])


def _check(out, want, rows, n_max, pairs, what):
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    exp = _expected(want, rows, n_max, pairs)
    if not ref.same_bits(got, exp):
        bits = np.uint16 if got.dtype == np.float16 else np.uint32
        with np.errstate(invalid="ignore"):
            bad = np.flatnonzero((got.view(bits) != exp.view(bits)) & ~(np.isnan(got) & np.isnan(exp)))
        pytest.fail("%s: %d of %d buffer elements differ, first at flat index %d (got %r, expected %r)"
                    % (what, bad.size, got.size, bad[0], got[bad[0]], exp[bad[0]]))


def _launch(kind, x, table, lv, n_max, n_dev, norm, pairs, out):
    """The `_ex` entry of a table kind; n_dev an int (placed on the device) or None (NULL)."""
    L = _lib()
    fn = {"f32": L.ngp_hash_fwd_f32_ex, "bf16": L.ngp_hash_fwd_bf16_ex, "f16": L.ngp_hash_fwd_f16_ex}[kind]
    cnt = None if n_dev is None else torch.tensor([n_dev], device=DEV, dtype=torch.int32)
    lo, hi = norm if norm is not None else (0.0, 1.0)
    rc = fn(_p(x), _p(table), ctypes.byref(lv), n_max, _p(cnt), int(norm is not None), float(lo), float(hi), pairs, _p(out), _stream())
    torch.cuda.synchronize()
    return rc


def _sweep(name, sizes, pairs, plain_f32=False):
    """Sizes of one case through its `_ex` entry (or, natural f32, the plain entry); the largest size twice: same bytes."""
    c, want, (x, table) = _case(name)
    for n in sizes:
        out = _buffer(n, want.shape[1])
        if plain_f32 and not pairs:
            assert _lib().ngp_hash_fwd_f32(_p(x), _p(table), ctypes.byref(c["lv"]), n, _p(out), _stream()) == 0
        else:
            assert _launch(c["kind"], x, table, c["lv"], n, None, c["norm"], pairs, out) == 0
        _check(out, want, slice(0, n), n, pairs, "%s n=%d pairs=%d" % (name, n, pairs))
    again = _buffer(n, want.shape[1])
    assert _launch(c["kind"], x, table, c["lv"], n, None, c["norm"], pairs, again) == 0
    assert torch.equal(out.view(torch.int32), again.view(torch.int32)), "second launch differs"


# ------------------------------------------------------------------------------------------------------- f32: sizes, layouts, tables
@pytest.mark.parametrize("pairs", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("name", ["c2_f32", "c3_f32"])
def test_f32_every_size(hip_lib, name, pairs):
    """One, two and three trips of the persistent grid, the tile edges 127 / 128 / 129 and the hand-over from the generic to the XCD
    kernel at 4095 / 4096 (natural layout; pair-major is the XCD kernel at every size)."""
    _sweep(name, SIZES_XCD, pairs, plain_f32=True)


@pytest.mark.parametrize("pairs", LAYOUTS, ids=LAYOUT_IDS)
def test_f32_real_modulo_table(hip_lib, pairs):
    """Hashed levels of 3 * 2^17 entries: the rarely taken branch that redoes a lane's eight indices with `%`."""
    _sweep("mod_f32", (129, ref.N_TRIPS2), pairs)


# ------------------------------------------------------------------------------------------------------------ the device-side count
@pytest.mark.parametrize("pairs", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("name,n_maxes", [("c2_f32", (5000, ref.N_TRIPS2)), ("c2_f16", (5000,)), ("c2_bf16", (5000,))])
def test_device_side_count(hip_lib, name, n_maxes, pairs):
    """Rows [n_dev, n_max) keep the fill on both layouts (the pair-major plane stride stays n_max), 0 writes nothing, a count above
    n_max encodes n_max rows."""
    c, want, (x, table) = _case(name)
    for n_max in n_maxes:
        for n_dev in (0, 1, 129, n_max - 1, n_max, n_max + 7):
            out = _buffer(n_max, 32)
            assert _launch(c["kind"], x, table, c["lv"], n_max, n_dev, None, pairs, out) == 0
            _check(out, want, slice(0, min(n_dev, n_max)), n_max, pairs, "%s n_max=%d n_dev=%d pairs=%d" % (name, n_max, n_dev, pairs))


@pytest.mark.parametrize("name", ["c2_f32", "g5f1_f32", "g5f4_f32", "g5f8_f32", "g5_bf16"])
def test_device_side_count_generic_kernel(hip_lib, name):
    """The same on the generic kernel (natural layout; 16 x 2 below 4096 rows, the 5-level tables of 1, 4 and 8 features and bf16)."""
    c, want, (x, table) = _case(name)
    n_max = 1000
    for n_dev in (0, 1, 129, n_max - 1, n_max, n_max + 7):
        out = _buffer(n_max, want.shape[1])
        assert _launch(c["kind"], x, table, c["lv"], n_max, n_dev, None, 0, out) == 0
        _check(out, want, slice(0, min(n_dev, n_max)), n_max, 0, "%s generic n_dev=%d" % (name, n_dev))


# ------------------------------------------------------------------------------------------------------------ fused normalisation
@pytest.mark.parametrize("name", sorted(k for k in ref.CASES if k.startswith("norm")))
def test_fused_normalisation(hip_lib, name):
    """(x - lo) / (hi - lo) inside the launch equals `normalise` then `forward32`, unclipped: the XCD kernel (n = 4097, and pair-major
    at n = 1000), whose power-of-two denominators take one multiply, and the generic kernel (n = 1000, natural), which divides."""
    c, want, (x, table) = _case(name)
    for n, pairs in ((4097, 0), (4097, 1), (1000, 0), (1000, 1)):
        out = _buffer(n, 32)
        assert _launch(c["kind"], x, table, c["lv"], n, None, c["norm"], pairs, out) == 0
        _check(out, want, slice(0, n), n, pairs, "%s n=%d pairs=%d" % (name, n, pairs))


# ------------------------------------------------------------------------------------------------------------------------- bf16
@pytest.mark.parametrize("pairs", LAYOUTS, ids=LAYOUT_IDS)
def test_bf16_every_size(hip_lib, pairs):
    _sweep("c2_bf16", (1, 129, 4095, 4096, ref.N_TRIPS2), pairs)


def test_bf16_generic_kernel_five_levels(hip_lib):
    _sweep("g5_bf16", (1, 255, 256, 257, 4097), 0)


# ---------------------------------------------------------------------------------------------------------------------- f16
@pytest.mark.parametrize("name", ["c2_f16", "g5_f16", "c3_f16"])
def test_f16_operator_kernel(hip_lib, name):
    """ngp_hash_fwd_f16: float16 output [n, L, 2]; 65 553 rows x 16 levels is the grid-stride second trip.  Bit equality on these
    ~10^7 products is also the guard against the compiler folding the product and its cast into one single-rounding instruction."""
    c = ref.case(name, _levels)
    want = ref.reference(c)
    _, _, (x, table) = _case(name)
    width = want.shape[1]
    for n in (1, 255, 256, 257, 65553):
        outs = []
        for _ in range(2 if n == 65553 else 1):
            out = _buffer(n, width, torch.float16)
            assert _lib().ngp_hash_fwd_f16(_p(x), _p(table), ctypes.byref(c["lv"]), n, _p(out), _stream()) == 0
            outs.append(out)
        _check(out, want, slice(0, n), n, 0, "%s operator n=%d" % (name, n))
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16))


@pytest.mark.parametrize("pairs", LAYOUTS, ids=LAYOUT_IDS)
def test_f16_ex_every_size(hip_lib, pairs):
    _sweep("c2_f16", (1, 129, ref.N_TRIPS2, ref.N_TRIPS3), pairs)


@pytest.mark.parametrize("pairs", LAYOUTS, ids=LAYOUT_IDS)
def test_f16_ex_fine_table(hip_lib, pairs):
    """Finest resolution 4096: rows INSIDE the box have cells above 2048, which float16 does not hold exactly, so the rounding of
    the cell before the subtract shows on ordinary rows (on the 1024 table only the rows outside the box reach such cells)."""
    _sweep("c3_f16", (129, ref.N_TRIPS2), pairs)


# ---------------------------------------------------------------------------------------------------------------------- list form
@pytest.mark.parametrize("pairs", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("name", ["list_f32", "list_bf16"])
def test_list_form(hip_lib, name, pairs):
    """Rows list[0 .. n) of a 200 000-row buffer, normalisation on: a shuffled strict subset, the identity and the reverse order, up to
    three trips -- the length at which the three-deep rotation of list entries has consumed every slot.  Rows outside the list keep
    the fill."""
    c, want, (x, table) = _case(name)
    L, n_max = _lib(), ref.N_LIST
    rng = np.random.default_rng(5)
    last = None
    for n in (0, 1, 127, 128, 129, ref.N_TRIPS2, ref.N_TRIPS3):
        lists = {"shuffled": rng.permutation(n_max)[:max(n, 1)], "identity": np.arange(max(n, 1)), "reverse": np.arange(max(n, 1))[::-1]}
        for order, rows in lists.items():
            rows = np.ascontiguousarray(rows, dtype=np.int32)
            lst, cnt = torch.from_numpy(rows).to(DEV), torch.tensor([n], device=DEV, dtype=torch.int32)
            out = _buffer(n_max, 32)
            assert L.ngp_hash_fwd_list(_p(x), _p(table), int(c["kind"] == "bf16"), ctypes.byref(c["lv"]), n_max, _p(cnt), _p(lst), 1,
                                       float(c["norm"][0]), float(c["norm"][1]), pairs, _p(out), _stream()) == 0
            _check(out, want, rows[:n].astype(np.int64), n_max, pairs, "%s %s n=%d pairs=%d" % (name, order, n, pairs))
            if order == "shuffled":
                last = (lst, cnt, out)
    lst, cnt, out = last
    again = _buffer(n_max, 32)
    assert L.ngp_hash_fwd_list(_p(x), _p(table), int(c["kind"] == "bf16"), ctypes.byref(c["lv"]), n_max, _p(cnt), _p(lst), 1,
                               float(c["norm"][0]), float(c["norm"][1]), pairs, _p(again), _stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), again.view(torch.int32))


# ------------------------------------------------------------------------------------------------------------------ generic kernel
@pytest.mark.parametrize("F", [1, 2, 4, 8])
def test_generic_kernel_every_feature_count(hip_lib, F):
    """Five levels (two dense, three hashed) of F features; F = 1 also at 209 800 rows, the grid-stride second trip."""
    _sweep("g5f%d_f32" % F, (1, 255, 256, 257, 4097) + ((209800,) if F == 1 else ()), 0)


# ------------------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_output_untouched(hip_lib):
    L = _lib()
    c, _, (x, table) = _case("c2_f32")
    _, _, (_, table16) = _case("c2_f16")
    lv16, lv5, lv3 = c["lv"], _levels(*ref.SHAPES["g5f2"]), _levels(2**14, 5, 8, 300, 3)
    out = _buffer(256, 32)
    cnt, lst = torch.tensor([4], device=DEV, dtype=torch.int32), torch.arange(4, device=DEV, dtype=torch.int32)
    s, null = _stream(), ctypes.c_void_p(0)
    assert L.ngp_hash_fwd_f32_ex(_p(x), _p(table), ctypes.byref(lv5), 256, null, 0, 0.0, 1.0, 1, _p(out), s) == -1     # pair-major, L != 16
    assert L.ngp_hash_fwd_bf16_ex(_p(x), _p(table), ctypes.byref(lv5), 256, null, 0, 0.0, 1.0, 1, _p(out), s) == -1
    assert L.ngp_hash_fwd_f16_ex(_p(x), _p(table16), ctypes.byref(lv5), 256, null, 0, 0.0, 1.0, 0, _p(out), s) == -1    # _f16_ex, L != 16
    assert L.ngp_hash_fwd_f32_ex(_p(x), _p(table), ctypes.byref(lv3), 256, null, 0, 0.0, 1.0, 0, _p(out), s) == -1     # F = 3
    assert L.ngp_hash_fwd_f32(_p(x), _p(table), ctypes.byref(lv3), 256, _p(out), s) == -1
    assert L.ngp_hash_fwd_list(_p(x), _p(table), 0, ctypes.byref(lv16), 256, _p(cnt), null, 0, 0.0, 1.0, 0, _p(out), s) == -1   # NULL list
    assert L.ngp_hash_fwd_list(_p(x), _p(table), 0, ctypes.byref(lv16), 256, null, _p(lst), 0, 0.0, 1.0, 0, _p(out), s) == -1
    assert L.ngp_hash_fwd_list(_p(x), _p(table), 0, ctypes.byref(lv5), 256, _p(cnt), _p(lst), 0, 0.0, 1.0, 0, _p(out), s) == -2  # other shape
    for n_max in (0, -5):
        assert L.ngp_hash_fwd_f32_ex(_p(x), _p(table), ctypes.byref(lv16), n_max, null, 0, 0.0, 1.0, 0, _p(out), s) == 0
        assert L.ngp_hash_fwd_bf16_ex(_p(x), _p(table), ctypes.byref(lv16), n_max, null, 0, 0.0, 1.0, 1, _p(out), s) == 0
        assert L.ngp_hash_fwd_f16_ex(_p(x), _p(table16), ctypes.byref(lv16), n_max, null, 0, 0.0, 1.0, 0, _p(out), s) == 0
        assert L.ngp_hash_fwd_f16(_p(x), _p(table16), ctypes.byref(lv16), n_max, _p(out), s) == 0
        assert L.ngp_hash_fwd_list(_p(x), _p(table), 0, ctypes.byref(lv16), n_max, _p(cnt), _p(lst), 0, 0.0, 1.0, 0, _p(out), s) == 0
    torch.cuda.synchronize()
    assert bool((out.view(torch.int32) == torch.tensor(-7.0).view(torch.int32).item()).all())


# ------------------------------------------------------------------------------------------------- loop variants: a child process
CHILD_SIZES = (1, 127, 128, 129, 257, 1200)
CHILD_NORM = (-1.7, 2.9)


@pytest.fixture(scope="module")
def child_inputs(tmp_path_factory):
    """The child's input file and the references of its forms (1200 rows of the C2 table's three kinds; the list forms read
    un-normalised positions)."""
    n_max = max(CHILD_SIZES)
    want = {}
    tables = {}
    for kind in ("f32", "bf16", "f16"):
        c, w, _ = _case("c2_" + kind)
        want[kind], tables[kind] = w[:n_max], c["table"]
    c = ref.case("c2_f32", _levels)
    x = np.ascontiguousarray(c["x"][:n_max])
    x_list = ref.denormalise(x, *CHILD_NORM)
    for kind in ("f32", "bf16"):
        want["list_" + kind] = ref.forward32(ref.normalise(x_list, *CHILD_NORM), tables[kind], c["lv"], kind)
    perm = np.random.default_rng(9).permutation(n_max).astype(np.int32)
    path = str(tmp_path_factory.mktemp("hash_forward_child") / "in.npz")
    np.savez(path, shape=np.array(ref.SHAPES["c2"]), x=x, x_list=x_list, lo_hi=np.array(CHILD_NORM), perm=perm,
             sizes=np.array(CHILD_SIZES), table_f32=tables["f32"], table_bf16=tables["bf16"], table_f16=tables["f16"])
    return path, want, perm


@pytest.mark.parametrize("setting,forms", [("hash_fwd_tiles=1", "f32,bf16,f16,list_f32,list_bf16"),
                                           ("hash_fwd_tiles=3", "f32,bf16,f16,list_f32,list_bf16"),
                                           ("hash_fwd_v1=1", "f32,bf16,f16"),       # the list form has no V1 loop (it returns -2)
                                           ("hash_fwd_v1=1;hash_fwd_tiles=1", "f32,bf16,f16")])
def test_loop_variants_in_a_child_process(hip_lib, child_inputs, tmp_path, setting, forms):
    """One tile: a lane takes ceil(n / 128) trips, ten at n = 1200, so the prefetch, the deferred store and the list rotation run
    their steady state at a size where the reference is instant.  Three tiles: strides that are no power of two.  V1: the loop tables
    of 4 GB and more take -- alone it keeps the cap of 768 tiles, so every lane makes one trip; with one tile it makes up to ten.
    One child at a time; a child that exits non-zero, dies by a signal or runs into the time limit fails the test and no further
    one starts."""
    if _child_died:
        pytest.fail("not started: the child for %s died" % _child_died[0])
    path, want, perm = child_inputs
    path_out = str(tmp_path / "out.npz")
    env = dict(os.environ, NGP_EXPERIMENT=setting)
    try:
        run = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "hash_forward_child.py"), path, path_out, forms], env=env,
                             capture_output=True, text=True, timeout=300)
    except subprocess.TimeoutExpired:
        _child_died.append(setting)
        pytest.fail("child (%s) did not finish within its time limit" % setting)
    if run.returncode != 0:
        _child_died.append(setting)
        pytest.fail("child (%s) exited with %d\n%s%s" % (setting, run.returncode, run.stdout[-2000:], run.stderr[-2000:]))
    got = np.load(path_out)
    n_max = max(CHILD_SIZES)
    for form in forms.split(","):
        for pairs in (0, 1):
            for n in CHILD_SIZES:
                out = got["%s_%d_%d" % (form, pairs, n)]
                if form.startswith("list_"):
                    exp = _expected(want[form], perm[:n].astype(np.int64), n_max, pairs)
                else:
                    exp = _expected(want[form], slice(0, n), n, pairs)
                assert ref.same_bits(out, exp), "%s: %s pairs=%d n=%d" % (setting, form, pairs, n)
