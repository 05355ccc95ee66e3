"""CPU tier of the hash encoder's position gradient: the numpy reference (tests/hash_input_grad_reference.py) is pinned to the corner
rule the project already pins to the reference, its analytic gradient is checked by central differences and by a hand-computed
case, and the three C-ABI entries are declared and bound."""
import os
import re

import numpy as np

from conftest import ROOT
import hash_input_grad_reference as ref

LEVELS_DEFAULT = (2**19, 16, 16, 2048, 2)
LEVELS_TINY = (2**10, 2, 4, 64, 2)           # a dense level (5^3 <= 128 entries) and a hashed one of 1024


def _points(n, seed):
    rng = np.random.default_rng(seed)
    return rng.random((n, 3), dtype=np.float32)


def test_reference_matches_the_pinned_corner_rule(oracle):
    """Corner entries equal, forward weights bit for bit, and the float64 forward within 1e-6 * sum |w * T| of the float32 one."""
    edge = np.array([[0, 0, 0], [1, 1, 1], [0.5, 0.5, 0.5], [1e-7, 1e-7, 1e-7], [0.999999, 0.999999, 0.999999],
                     [1.25, -0.25, 3.0], [1024.0 / 2047.0, 0.25, 0.75]], dtype=np.float32)
    for shape in (LEVELS_DEFAULT, LEVELS_TINY, (2**21, 4, 32, 128, 4), (2**14, 5, 8, 300, 1)):
        lv = oracle.make_levels(*shape)
        x = np.concatenate([edge, _points(500, 1)])
        idx, w = ref.corners(x, lv)
        idx_o, w_o = oracle.hash_corners(x, lv)
        assert np.array_equal(idx, idx_o)
        assert np.array_equal(w.view(np.uint32), w_o.view(np.uint32))
        table = np.random.default_rng(2).standard_normal(lv.total_entries * lv.n_features).astype(np.float32)
        enc, mag = ref.forward64(x, table, lv)
        enc_o = oracle.hash_fwd_f32(x, table, lv)
        assert np.all(np.abs(enc - enc_o) <= 1e-6 * mag + 1e-30)


def test_tiny_table_has_a_dense_a_hashed_and_a_modulo_level(oracle):
    """The GPU tests' tiny table exercises what its comment says: level 0 dense, level 1 hashed; and max_params 1000 (no power of
    two) gives a hashed level that takes the real modulo."""
    t = ref.level_table(oracle.make_levels(*LEVELS_TINY))
    assert t["bfhl"] == 1 and t["res"][0] ** 3 <= t["size"][0] and t["res"][1] ** 3 > t["size"][1]
    t = ref.level_table(oracle.make_levels(1000, 2, 4, 64, 2))
    assert t["bfhl"] == 1 and t["size"][1] == 1000


def test_central_differences(oracle):
    """All in float64 with float64 cells: inside a cell the encoding is linear along one axis, so central differences with a step
    that stays inside every level's cell reproduce the analytic gradient to 1e-9 * S."""
    lv = oracle.make_levels(*LEVELS_DEFAULT)
    t = ref.level_table(lv)
    rng = np.random.default_rng(3)
    x = rng.random((4096, 3))
    keep = np.ones(len(x), dtype=bool)
    for l in range(t["L"]):
        _, fr = ref.cell_frac(x, t["scale"][l], exact=True)
        keep &= np.all((fr >= 0.02) & (fr <= 0.98), axis=1)
    x = x[keep]
    print("central differences: %d of 4096 points survive the fraction filter" % len(x))
    assert len(x) >= 256
    table = rng.standard_normal(lv.total_entries * 2)
    denc = rng.standard_normal((len(x), 32))
    dx, S = ref.grad64(x, table, denc, lv, exact=True)
    h = 0.005 / float(t["scale"][-1])
    worst = 0.0
    for k in range(3):
        e = np.zeros(3)
        e[k] = h
        fp, _ = ref.forward64(x + e, table, lv, exact=True)
        fm, _ = ref.forward64(x - e, table, lv, exact=True)
        fd = ((fp - fm) * denc).sum(1) / (2 * h)
        worst = max(worst, float(np.max(np.abs(fd - dx[:, k]) / S[:, k])))
        assert np.all(np.abs(fd - dx[:, k]) <= 1e-9 * S[:, k])
    print("central differences: worst |fd - dx| / S = %.3g" % worst)


def test_hand_case_linear_table():
    """One dense level of 8^3 grid points whose table is slope * gy + c: dx = scale * slope * denc along y and 0 along x and z."""
    from ngp_hip.lib import HashLevels
    lv = HashLevels()
    lv.n_levels, lv.n_features, lv.begin_fast_hash_level, lv.total_entries = 1, 1, 1, 512
    lv.scale[0], lv.resolution[0], lv.map_size[0], lv.offset[0] = 7.0, 8, 512, 0
    slope, c = 0.375, -2.0
    g = np.arange(8)
    table = np.broadcast_to((slope * g + c)[None, :, None], (8, 8, 8)).reshape(-1).astype(np.float32)   # entry gx + 8 gy + 64 gz
    x = (_points(64, 4) * np.float32(0.85)).astype(np.float32)
    denc = np.random.default_rng(5).standard_normal((64, 1)).astype(np.float32)
    want = np.zeros((64, 3))
    want[:, 1] = 7.0 * slope * denc[:, 0].astype(np.float64)
    for half in (False, True):
        dx, S = ref.grad64(x, table, denc, lv, half=half)
        assert np.all(np.abs(dx - want) <= 1e-6 * S)
        dx32 = ref.grad32(x, table, denc, lv, half=half)
        assert np.all(np.abs(dx32 - want) <= 1e-5 * S)


def test_serial_float32_tracks_float64(oracle):
    """grad32 is an independent evaluation of the formula: it agrees with grad64 to float32 rounding of a 256-term sum."""
    lv = oracle.make_levels(*LEVELS_DEFAULT)
    rng = np.random.default_rng(6)
    x = _points(300, 7)
    table = rng.standard_normal(lv.total_entries * 2).astype(np.float32)
    denc = rng.standard_normal((300, 32)).astype(np.float32)
    for half in (False, True):
        dx, S = ref.grad64(x, table, denc, lv, half=half)
        dx32 = ref.grad32(x, table, denc, lv, half=half)
        e32 = float(np.max(np.abs(dx32 - dx) / S))
        print("half=%s: E32 = %.3g" % (half, e32))
        assert 0 < e32 < (256 + 8) * 2.0**-24          # worst case of a 256-term float32 sum with ~8 roundings per term


def test_entries_declared_and_bound():
    """ngp_hash_bwd_input_{f32,bf16,f16} are part of the boundary header (not the experimental one) and of the ctypes table."""
    from ngp_hip import lib
    hdr = open(os.path.join(ROOT, "include", "ngp_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("ngp_hash_bwd_input_f32", "ngp_hash_bwd_input_bf16", "ngp_hash_bwd_input_f16"):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in lib.SIGNATURES and name not in lib.EXPERIMENTAL
        assert len(lib.SIGNATURES[name]) == 7
    assert "hash_grad_input.hip" in lib.SOURCES
