"""CPU tier of the hash encoder's double backward: the float64 reference (tests/hash_input_grad2_reference.py) is checked by central
differences of the first-order reference, by its two exact zeros and against torch's own double backward of a plain-torch encoder,
and the three C-ABI entries are declared and bound."""
import os
import re

import numpy as np
import torch

from conftest import ROOT
import hash_input_grad_reference as ref
import hash_input_grad2_reference as ref2

LEVELS_DEFAULT = (2**19, 16, 16, 2048, 2)
LEVELS_TINY = (2**10, 2, 4, 64, 2)


def test_central_differences(oracle):
    """Phi_i = ddx_i . dx_i (dx from grad64, all in float64 with float64 cells) is linear in every table entry and in denc, and inside
    a cell linear in each coordinate: central differences of Phi reproduce d_table, d_denc and d_x to 1e-9 * S.  The same point filter
    and seed as test_hash_input_grad.test_central_differences."""
    lv = oracle.make_levels(*LEVELS_DEFAULT)
    t = ref.level_table(lv)
    rng = np.random.default_rng(3)
    x = rng.random((4096, 3))
    keep = np.ones(len(x), dtype=bool)
    for l in range(t["L"]):
        _, fr = ref.cell_frac(x, t["scale"][l], exact=True)
        keep &= np.all((fr >= 0.02) & (fr <= 0.98), axis=1)
    x = x[keep]
    n = len(x)
    assert n >= 256
    table = rng.standard_normal(lv.total_entries * 2)
    denc = rng.standard_normal((n, 32))
    ddx = rng.standard_normal((n, 3))
    d_denc, S_denc, d_x, S_x, d_table, S_table = ref2.bwd2_64(x, table, denc, ddx, lv, exact=True)

    def phi(x_, table_, denc_):
        dx, _ = ref.grad64(x_, table_, denc_, lv, exact=True)
        return (dx * ddx).sum(1)                                   # per sample: a perturbation reaches only the samples it touches

    # denc: one column at a time, every sample at once (the samples are independent)
    worst = 0.0
    for e in range(32):
        step = np.zeros((1, 32))
        step[0, e] = 1.0
        fd = (phi(x, table, denc + step) - phi(x, table, denc - step)) / 2.0
        worst = max(worst, float(np.max(np.abs(fd - d_denc[:, e]) / S_denc[:, e])))
        assert np.all(np.abs(fd - d_denc[:, e]) <= 1e-9 * S_denc[:, e])
    print("central differences: worst |fd - d_denc| / S = %.3g" % worst)

    # x: the step stays inside every level's cell
    h = 0.005 / float(t["scale"][-1])
    worst = 0.0
    for m in range(3):
        e = np.zeros(3)
        e[m] = h
        fd = (phi(x + e, table, denc) - phi(x - e, table, denc)) / (2 * h)
        worst = max(worst, float(np.max(np.abs(fd - d_x[:, m]) / S_x[:, m])))
        assert np.all(np.abs(fd - d_x[:, m]) <= 1e-9 * S_x[:, m])
    print("central differences: worst |fd - d_x| / S = %.3g" % worst)

    # table: two corner entries of every level (both features) and one entry no sample touches
    idx, _ = ref.corners(x.astype(np.float32), lv)                 # float32 cells: only used to pick entries, any entry serves
    picks = []
    for l in range(t["L"]):
        picks += [int(idx[5, l, 0]) * 2, int(idx[n // 2, l, 7]) * 2 + 1]
    untouched = int(np.flatnonzero(S_table == 0)[0])
    worst = 0.0
    for p in picks + [untouched]:
        old = table[p]
        table[p] = old + 1.0
        hi = phi(x, table, denc)
        table[p] = old - 1.0
        lo = phi(x, table, denc)
        table[p] = old
        fd = float(((hi - lo) / 2.0).sum())
        assert abs(fd - d_table[p]) <= 1e-9 * S_table[p], (p, fd, d_table[p], S_table[p])
        if S_table[p] > 0:
            worst = max(worst, abs(fd - d_table[p]) / S_table[p])
    assert sum(S_table[p] > 0 for p in picks) >= 16                # most picks are entries the filtered points really touch
    print("central differences: worst |fd - d_table| / S = %.3g" % worst)


def _random_input(oracle, shape, n, seed):
    lv = oracle.make_levels(*shape)
    rng = np.random.default_rng(seed)
    x = rng.random((n, 3), dtype=np.float32)
    table = rng.standard_normal(lv.total_entries * lv.n_features).astype(np.float32)
    denc = rng.standard_normal((n, lv.n_levels * lv.n_features)).astype(np.float32)
    ddx = rng.standard_normal((n, 3)).astype(np.float32)
    return lv, x, table, denc, ddx


def test_unit_ddx_leaves_its_own_axis_alone(oracle):
    """The diagonal of the second derivative is exactly 0: ddx = e_k gives d_x[:, k] == 0, in float64 and in the serial float32."""
    lv, x, table, denc, _ = _random_input(oracle, LEVELS_DEFAULT, 200, 11)
    for k in range(3):
        ddx = np.zeros((200, 3), dtype=np.float32)
        ddx[:, k] = 1.0
        _, _, d_x, S_x, _, _ = ref2.bwd2_64(x, table, denc, ddx, lv)
        _, d_x32, _ = ref2.bwd2_32(x, table, denc, ddx, lv)
        assert np.all(d_x[:, k] == 0) and np.all(S_x[:, k] == 0) and np.all(d_x32[:, k] == 0)
        others = [m for m in range(3) if m != k]
        assert np.all(d_x[:, others] != 0)


def test_constant_table_gives_zero_d_denc(oracle):
    """A table that is constant over the cell: every corner difference is exactly 0, so d_denc == 0 exactly (S_denc is not)."""
    lv, x, table, denc, ddx = _random_input(oracle, LEVELS_DEFAULT, 200, 12)
    table[:] = 0.75
    d_denc, S_denc, _, _, _, _ = ref2.bwd2_64(x, table, denc, ddx, lv)
    assert np.all(d_denc == 0) and np.all(S_denc > 0)


def test_torch_double_backward_equals_the_reference(oracle):
    """torch's autograd, twice, through the plain-torch float64 encoder gives what bwd2_64 writes out by hand, to 1e-12 * S; its
    float32 instance tracks it to float32 rounding."""
    for shape, n in ((LEVELS_TINY, 300), (LEVELS_DEFAULT, 200)):
        lv, x, table, denc, ddx = _random_input(oracle, shape, n, 13)
        d_denc, S_denc, d_x, S_x, d_table, S_table = ref2.bwd2_64(x, table, denc, ddx, lv)
        dx64, S = ref.grad64(x, table, denc, lv)
        for dtype, rel in ((torch.float64, 1e-12), (torch.float32, (16 * 8 * 2 * 4 + 8) * 2.0**-24)):
            xt = torch.from_numpy(x).to(dtype).requires_grad_()
            tt = torch.from_numpy(table).to(dtype).requires_grad_()
            gt = torch.from_numpy(denc).to(dtype).requires_grad_()
            enc = ref2.TorchEncoder(lv, dtype)(xt, tt)
            (gx,) = torch.autograd.grad((enc * gt).sum(), xt, create_graph=True)
            assert np.all(np.abs(gx.detach().double().numpy() - dx64) <= rel * S)
            (gx * torch.from_numpy(ddx).to(dtype)).sum().backward()
            assert np.all(np.abs(gt.grad.double().numpy() - d_denc) <= rel * S_denc)
            assert np.all(np.abs(xt.grad.double().numpy() - d_x) <= rel * S_x)
            assert np.all(np.abs(tt.grad.double().numpy() - d_table) <= rel * S_table)
            assert tt.grad.dtype == dtype


def test_serial_float32_tracks_float64(oracle):
    """bwd2_32 is an independent evaluation of the three formulas: it agrees with bwd2_64 to float32 rounding of its longest sum."""
    lv, x, table, denc, ddx = _random_input(oracle, LEVELS_DEFAULT, 300, 14)
    d_denc, S_denc, d_x, S_x, d_table, S_table = ref2.bwd2_64(x, table, denc, ddx, lv)
    d_denc32, d_x32, d_table32 = ref2.bwd2_32(x, table, denc, ddx, lv)
    touched = S_table > 0
    assert np.all(d_table32[~touched] == 0) and np.all(d_table[~touched] == 0)
    for name, a, b, S in (("d_denc", d_denc32, d_denc, S_denc), ("d_x", d_x32, d_x, S_x),
                          ("d_table", d_table32[touched], d_table[touched], S_table[touched])):
        e32 = float(np.max(np.abs(a - b) / S))
        print("%s: E32 = %.3g" % (name, e32))
        assert 0 < e32 < (16 * 8 * 2 * 4 + 8) * 2.0**-24     # d_x: 16 levels x 8 corners x 2 features x 4 terms, ~8 roundings per term


def test_entries_declared_and_bound():
    """ngp_hash_bwd2_{gather_f32,gather_bf16,table_f32} are part of the boundary header (not the experimental one) and of the ctypes
    table, and their source is part of the build."""
    from ngp_hip import lib
    hdr = open(os.path.join(ROOT, "include", "ngp_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, n_args in (("ngp_hash_bwd2_gather_f32", 9), ("ngp_hash_bwd2_gather_bf16", 9), ("ngp_hash_bwd2_table_f32", 7)):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in lib.SIGNATURES and name not in lib.EXPERIMENTAL
        assert len(lib.SIGNATURES[name]) == n_args
    assert "hash_grad_input2.hip" in lib.SOURCES
