"""Hand-derived known answers (tests/golden/kat_hand.json: every expected value follows from the reference's formulas by integer or
exact dyadic arithmetic, none was produced by running code) held against THREE implementations alike:

  * `shim`   -- the reference's own kernel source (its modules/*.py) executed under oracle/ti_shim: the thing the golden fixtures
                come from, here pinned against something that is not itself (CPU).  Where the reference checkout exists the shim runs
                here and must reproduce tests/golden/ref_kat_shim.npz (oracle/gen_golden_checkout.py); elsewhere that file is read, and
                the `test_shim_*` tests are a consistency check of the two fixtures, not a run of the shim;
  * `oracle` -- the C restatement (CPU, everywhere);
  * `hip`    -- the product kernels through the C ABI (`-m gpu`).
Plus the notebook regime: the shim-executed march reproduces the sample density a real Taichi run of the reference printed
(notebooks/pipeline.ipynb cells 12-14) within the stated tolerance, and oracle / HIP reproduce the shim's per-ray counts exactly.
"""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

KAT = json.load(open(os.path.join(GOLDEN, "kat_hand.json")))
HAVE_REF = os.path.exists("/root/reference/modules/hash_encoder.py")


@pytest.fixture(scope="module")
def shim_out():
    """The shim's outputs on the KAT inputs: computed from the reference checkout where it exists (and held to the stored fixture),
    the stored fixture elsewhere."""
    stored = dict(np.load(os.path.join(GOLDEN, "ref_kat_shim.npz")))
    if not HAVE_REF:
        return stored
    import sys
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(here, "oracle"))
    from gen_golden import load_reference
    from gen_golden_checkout import shim_kat_outputs
    live = shim_kat_outputs(load_reference())
    assert set(live) == set(stored)
    for k in live:
        assert live[k].dtype == stored[k].dtype and np.array_equal(live[k], stored[k], equal_nan=live[k].dtype.kind == "f"), k
    return live


def _table_for(entries, n_floats):
    t = np.zeros(n_floats, np.float32)
    for k, (f0, f1) in entries.items():
        t[2 * int(k)], t[2 * int(k) + 1] = f0, f1
    return t


def _hash_cases():
    """(name, x [1,3], table, level, expected [2], exact?)"""
    n_floats = 5710032 * 2
    k = KAT["hash_level0_trilinear"]
    yield "level0_trilinear", np.array([k["x"]], np.float32), _table_for(k["table_entries"], n_floats), k["level"], k["expected"], True
    c = KAT["hash_lattice_corner"]
    for case in c["cases"]:
        yield ("lattice_l%d_%s" % (case["level"], "_".join(map(str, case["cell"]))), np.array([case["x"]], np.float32),
               _table_for({case["entry"]: c["feature"]}, n_floats), case["level"], c["feature"], case["exact"])


def _check_hash(out, level, want, exact, name=""):
    got = out[0, 2 * level:2 * level + 2].tolist()
    if exact:
        assert got == want, (name, got)
    else:               # (scale of this level = f32 exp(): one ulp between implementations, see the case's note)
        np.testing.assert_allclose(got, want, rtol=1e-4, err_msg=name)
    assert np.all(np.delete(np.asarray(out[0]), [2 * level, 2 * level + 1]) == 0), name      # every other level reads zeros


# ------------------------------------------------------------------------------------------------------------ oracle
def test_oracle_scalar_kats(oracle):
    for x, e in KAT["frexp_bit"]["cases"]:
        assert oracle.frexp_bit(x) == e, x
    pts = np.array([c for c, _ in KAT["morton3d"]["cases"]], np.int32)
    assert oracle.morton3d(pts).tolist() == [m for _, m in KAT["morton3d"]["cases"]]
    assert np.array_equal(oracle.morton3d_invert(np.array([m for _, m in KAT["morton3d"]["cases"]], np.int32)), pts)
    pk = KAT["packbits"]
    assert oracle.packbits(np.array(pk["grid"], np.float32), pk["threshold"]).tolist() == [pk["byte"]]


@pytest.mark.parametrize("case", list(_hash_cases()), ids=lambda c: c[0])
def test_oracle_hash_kats(oracle, case):
    name, x, table, level, want, exact = case
    lv = oracle.make_levels(2**19, 16, 16, 1024, 2)
    _check_hash(oracle.hash_fwd_f32(x, table, lv), level, want, exact, name)


def _composite_inputs():
    c = KAT["composite_two_rays"]
    return (np.array(c["sigmas"], np.float32), np.array(c["rgbs"], np.float32), np.array(c["deltas"], np.float32),
            np.array(c["ts"], np.float32), np.array(c["rays_a"], np.int32), c["T_threshold"], c["expected"])


def _check_composite(total, op, dep, rgb, ws, want):
    assert list(map(int, total)) == want["total_samples"]
    assert list(map(float, op)) == want["opacity"] and list(map(float, dep)) == want["depth"]
    assert np.asarray(rgb, np.float32).tolist() == np.asarray(want["rgb"], np.float32).tolist()
    for got, w in zip(ws, want["ws_composited"]):
        if w is not None:                                          # (samples behind the termination point: uninitialised in the reference)
            assert float(got) == w


def test_oracle_composite_kat(oracle):
    s, c, dl, t, ra, thr, want = _composite_inputs()
    total, op, dep, rgb, ws = oracle.composite_train_fwd(s, c, dl, t, ra, thr)
    _check_composite(total, op, dep, rgb, ws, want)


def test_oracle_level_table_is_the_notebooks(oracle):
    nb = KAT["level_table_notebook"]
    lv = oracle.make_levels(2**19, 16, 16, 1024, 2)
    assert lv.total_entries == nb["offset"] and lv.total_entries * lv.n_features == nb["total_hash_size"]
    # per_level_scale = exp(log_b) with log_b = ln(1024 / 16) / 15 in f64 (utils.py:31-39)
    assert abs(np.exp(np.log(1024.0 / 16.0) / 15.0) - nb["per_level_scale"]) < 1e-12


# ------------------------------------------------------------------------------------------------------------ shim (reference source)
def test_shim_scalar_kats(shim_out):
    """The shim's frexp_bit / morton3D / packbits against the KATs.  Without the reference checkout no shim code runs: this is then a
    consistency check of two fixtures (the stored shim outputs, ref_kat_shim.npz, against kat_hand.json)."""
    for (x, e), got in zip(KAT["frexp_bit"]["cases"], shim_out["frexp_bit"]):
        assert int(got) == e, x
    assert len(shim_out["frexp_bit"]) == len(KAT["frexp_bit"]["cases"])
    assert [int(v) for v in shim_out["morton3d"]] == [m for _, m in KAT["morton3d"]["cases"]]
    assert [int(v) for v in shim_out["packbits"]] == [KAT["packbits"]["byte"]]


@pytest.mark.parametrize("case", list(_hash_cases()), ids=lambda c: c[0])
def test_shim_hash_kats(shim_out, case):
    """The shim's hash encoder against the KATs (without the checkout: stored shim outputs against kat_hand.json, fixture consistency)."""
    name, x, table, level, want, exact = case
    _check_hash(shim_out["hash__" + name], level, want, exact, name)


def test_shim_composite_kat(shim_out):
    """The shim's training composite against the KAT (without the checkout: stored shim outputs against kat_hand.json, fixture
    consistency)."""
    _, _, _, _, _, _, want = _composite_inputs()
    _check_composite(shim_out["composite_total"], shim_out["composite_opacity"], shim_out["composite_depth"], shim_out["composite_rgb"],
                     shim_out["composite_ws"], want)


def _regime():
    return np.load(os.path.join(GOLDEN, "ref_notebook_regime.npz"))


def _regime_inputs(g):
    from ngp_hip import synthetic
    n = int(g["n_rays"])
    o, d = synthetic.lego_rays(n, seed=int(g["ray_seed"]))
    bits = synthetic.random_bitfield(1, 128, 0.5, seed=int(g["bits_seed"]))
    noise = np.random.default_rng(int(g["noise_seed"])).random(n, dtype=np.float32)
    return o, d, bits, noise


def test_shim_march_reproduces_the_notebooks_sample_density():
    """The fixture was made by the reference's march kernel under the shim; its samples per ray sit within the stated tolerance of
    what the notebook's real-Taichi run printed (2 055 705 samples / 8192 rays)."""
    g, nb = _regime(), KAT["march_notebook_regime"]
    per_ray = int(g["total"]) / int(g["n_rays"])
    want = nb["samples"] / nb["rays"]
    assert int(g["counts"].sum()) == int(g["total"])
    assert abs(per_ray - want) <= nb["tolerance_relative"] * want, (per_ray, want)
    lt = KAT["level_table_notebook"]
    assert abs(float(g["per_level_scale"]) - lt["per_level_scale"]) < 1e-12 and int(g["total_param_size"]) == lt["total_hash_size"]
    assert int(g["offsets"][-1] + g["hash_map_sizes"][-1]) == lt["offset"]


def test_oracle_reproduces_the_shims_march_in_that_regime(oracle):
    g = _regime()
    o, d, bits, noise = _regime_inputs(g)
    hits = oracle.ray_aabb(o, d, 0.5)
    assert np.array_equal(hits.view(np.uint32), g["hits_t"].view(np.uint32))
    rays_a, xyzs, dirs, deltas, ts, total = oracle.march_train(o, d, hits, bits, noise, 1, 0.5, 0.0, 128, 1024)
    assert total == int(g["total"]) and np.array_equal(rays_a[:, 2], g["counts"])
    has = rays_a[:, 2] > 0
    first, last = rays_a[:, 1], rays_a[:, 1] + rays_a[:, 2] - 1
    assert np.array_equal(ts[first[has]].view(np.uint32), g["t_first"][has].view(np.uint32))
    assert np.array_equal(ts[last[has]].view(np.uint32), g["t_last"][has].view(np.uint32))
    assert np.array_equal(deltas[first[has]].view(np.uint32), g["dt_first"][has].view(np.uint32))
    assert float(ts.astype(np.float64).sum()) == float(g["ts_sum"])
    lv = oracle.make_levels(2**19, 16, 16, 1024, 2)
    assert list(lv.offset[:16]) == g["offsets"].tolist() and list(lv.map_size[:16]) == g["hash_map_sizes"].tolist()
    assert lv.begin_fast_hash_level == int(g["begin_fast_hash_level"])


# ------------------------------------------------------------------------------------------------------------ HIP
@pytest.mark.gpu
def test_hip_kats(hip_lib):
    from ngp_hip import ops
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    pts = np.array([c for c, _ in KAT["morton3d"]["cases"]], np.int32)
    codes = [m for _, m in KAT["morton3d"]["cases"]]
    assert ops.morton3d(dev(pts)).cpu().tolist() == codes
    assert np.array_equal(ops.morton3d_invert(dev(np.array(codes, np.int32))).cpu().numpy(), pts)
    pk = KAT["packbits"]
    bits = torch.zeros(1, dtype=torch.uint8, device="cuda")
    ops.packbits(dev(np.array(pk["grid"], np.float32)), pk["threshold"], bits)
    assert int(bits[0]) == pk["byte"]
    lv = ops.make_levels(2**19, 16, 16, 1024, 2)
    for name, x, table, level, want, exact in _hash_cases():
        _check_hash(ops.hash_fwd_f32(dev(x), dev(table), lv).cpu().numpy(), level, want, exact, name)
    s, c, dl, t, ra, thr, want = _composite_inputs()
    total, op, dep, rgb, ws = ops.composite_train_fwd(dev(s), dev(c), dev(dl), dev(t), dev(ra), thr)
    _check_composite(total.cpu().numpy(), op.cpu().numpy(), dep.cpu().numpy(), rgb.cpu().numpy(), ws.cpu().numpy(), want)


@pytest.mark.gpu
def test_hip_reproduces_the_shims_march_in_that_regime(hip_lib):
    """frexp_bit / mip selection / the skip rule have no entry point of their own: they are held through the march (the fixture's
    per-ray counts and first / last samples, made by the reference's source under the shim)."""
    from ngp_hip import ops
    g = _regime()
    o, d, bits, noise = _regime_inputs(g)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    hits = ops.ray_aabb(dev(o), dev(d), 0.5)
    assert np.array_equal(hits.cpu().numpy().view(np.uint32), g["hits_t"].view(np.uint32))
    rays_a, xyzs, dirs, deltas, ts, total = ops.march_train(dev(o), dev(d), hits, dev(bits), dev(noise), 1, 0.5, 0.0, 128, 1024)
    ra, ts, deltas = rays_a.cpu().numpy(), ts.cpu().numpy(), deltas.cpu().numpy()
    assert int(total) == int(g["total"]) and np.array_equal(ra[:, 2], g["counts"])
    has = ra[:, 2] > 0
    first, last = ra[:, 1], ra[:, 1] + ra[:, 2] - 1
    assert np.array_equal(ts[first[has]].view(np.uint32), g["t_first"][has].view(np.uint32))
    assert np.array_equal(ts[last[has]].view(np.uint32), g["t_last"][has].view(np.uint32))
    assert np.array_equal(deltas[first[has]].view(np.uint32), g["dt_first"][has].view(np.uint32))
    assert float(ts[:int(total)].astype(np.float64).sum()) == float(g["ts_sum"])
