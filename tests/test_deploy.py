"""Deployment-model loader and the numpy restatement of its inference against the reference's own run (CPU tier).

tests/golden/ref_deploy.npz comes from scripts/gen_golden_deploy.py: the reference's deployment kernels (hash_encode, sigma_rgb_layer) on
per-sample rows and its run_inference on a 24x48 image, executed under oracle/ti_shim.  The tolerances of the sigma / rgb rows are
derived here from the fixture itself (its distance to the float64 restatement, times 4: profiles/PARITY_NOTES.md)."""
import os

import numpy as np
import pytest

import deploy_reference as dr
from conftest import GOLDEN


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(GOLDEN, "ref_deploy.npz")))


@pytest.fixture(scope="module")
def row_table(fx):
    return dr.synthetic_table(float(fx["rows_table_amplitude"]))


def fixture_levels(fx):
    """The level table with the scales the reference's kernel computed (its own f32 exp)."""
    _, res, size, offset = dr.level_table()
    return fx["level_scale"].astype(np.float32), res, size, offset


# ---------------------------------------------------------------------------------------------------- level table
def test_level_table_is_the_reference_initialize(hip_lib, oracle, fx):
    from ngp_hip import ops
    lv = ops.make_levels(2**21, 4, 32, 128, 4)
    scale, res, size, offset = ops.levels_to_numpy(lv)
    assert lv.total_entries == dr.TOTAL_ENTRIES == 2794024 and lv.begin_fast_hash_level == 4          # all four levels dense
    assert offset.tolist() == [0, 32768, 165424, 696872] == fx["offsets"].tolist()                      # kernels.py:initialize
    assert res.tolist() == [32, 51, 81, 128]
    assert (size.astype(np.int64) >= res.astype(np.int64)**3).all()
    s2, r2, z2, o2 = dr.level_table()
    assert np.array_equal(r2, res) and np.array_equal(z2, size) and np.array_equal(o2, offset)
    olv = oracle.make_levels(2**21, 4, 32, 128, 4)
    assert list(olv.offset[:4]) == offset.tolist() and list(olv.resolution[:4]) == res.tolist() and olv.total_entries == lv.total_entries
    # the scales: the library's expf, numpy's f32 exp and the reference's kernel (the shim's f32 exp) -- printed, compared bit for bit
    print("scales lib %s restatement %s reference %s" % (scale.view(np.uint32), s2.view(np.uint32), fx["level_scale"].view(np.uint32)))
    assert np.allclose(scale, fx["level_scale"], rtol=2e-7, atol=0)
    assert abs(float(fx["per_level_scale"]) - dr.LOG_B) <= 1e-6 * dr.LOG_B


# ---------------------------------------------------------------------------------------------------- restatement vs the reference
def test_rows_cover_the_cases(fx):
    x01 = fx["rows_xyz"] + np.float32(0.5)
    assert (x01 == 0).any(0).all() and (x01[:, :2] == 1).any(0).all()                                  # faces, x01 = 1 where in bounds
    n = np.linalg.norm(fx["rows_dirs"], axis=1)
    assert (n > 3).any() and (n < 0.3).any()                                                            # non-unit directions
    idx, size = dr.corner_indices(fx["rows_xyz"], dr.level_table())
    assert (idx < size[None, :, None]).all()                                                            # the reference stayed inside every level


def test_embedding_bit_exact(fx, row_table):
    enc = dr.embed(fx["rows_xyz"], row_table, fixture_levels(fx))
    assert np.array_equal(enc.view(np.uint32), fx["rows_enc"].view(np.uint32))


def _row_errors(fx, row_table, tag, dtype):
    enc = fx["rows_enc"] if dtype == np.float32 else dr.embed(fx["rows_xyz"], row_table, fixture_levels(fx), np.float64)
    _, sigma, rgb = dr.mlp(enc, fx["rows_dirs"], fx["sigma_weights_" + tag], fx["rgb_weights_" + tag], dtype)
    ref_s, ref_c = fx["rows_sigma_" + tag].astype(np.float64), fx["rows_rgb_" + tag].astype(np.float64)
    return np.abs(sigma / ref_s - 1).max(), np.abs(rgb - ref_c).max()


@pytest.mark.parametrize("tag", ["lego", "syn"])
def test_bounds_are_four_times_the_reference_error(fx, row_table, tag):
    """The bound of a sigma / rgb row is 4x the distance of the reference's own f32 result from the float64 restatement (whole graph in
    double from the f32 inputs).  deploy_reference.BOUNDS holds that product rounded up to two digits; this re-measures it."""
    es, ec = _row_errors(fx, row_table, tag, np.float64)
    bs, bc = dr.BOUNDS[tag]
    print("%s: reference vs f64: sigma rel %.3e rgb abs %.3e -> bounds %.3e %.3e" % (tag, es, ec, bs, bc))
    assert 4 * es <= bs <= 4 * es * 1.06 and 4 * ec <= bc <= 4 * ec * 1.06


@pytest.mark.parametrize("tag", ["lego", "syn"])
def test_restatement_rows(fx, row_table, tag):
    es, ec = _row_errors(fx, row_table, tag, np.float32)
    print("%s: f32 restatement vs reference: sigma rel %.3e rgb abs %.3e" % (tag, es, ec))
    assert np.isfinite(fx["rows_sigma_" + tag]).all() and (fx["rows_sigma_" + tag] > 0).all()
    assert es <= dr.BOUNDS[tag][0] and ec <= dr.BOUNDS[tag][1]


def test_restatement_image(fx, oracle, lego_bitfield):
    w, h = (int(v) for v in fx["img_res_wh"])
    table = dr.synthetic_table(float(fx["img_table_amplitude"]))
    rgb, opacity, _, schedule, total, state = dr.render_progressive(
        oracle, fx["pose"], dr.directions(w, h), lego_bitfield, table, fixture_levels(fx), fx["sigma_weights_syn"], fx["rgb_weights_syn"],
        float(fx["img_T_threshold"]), int(fx["img_max_samples"]))
    assert schedule == [tuple(r) for r in fx["img_schedule"].tolist()]
    assert total == int(fx["img_total_samples"])
    assert np.array_equal(np.flatnonzero(state == 2), fx["img_alive_at_end"])
    err_c, err_o = np.abs(rgb - fx["img_rgb"]).max(), np.abs(opacity - fx["img_opacity"]).max()
    print("image: rgb %.3e opacity %.3e" % (err_c, err_o))
    assert err_c <= 1e-3 and err_o <= 1e-3
    # the fixture is not degenerate (asserted by the generator on the reference's output; re-checked on the stored arrays)
    hit = fx["img_opacity"] > 0
    assert ((fx["img_opacity"] > 0.05) & (fx["img_opacity"] < 0.95)).sum() >= 0.1 * hit.sum()
    assert len(fx["img_alive_at_end"]) >= 1 and (state == 1).sum() >= 1


# ---------------------------------------------------------------------------------------------------- loaders
def _model_dict(rng, half_exact=True):
    """A deployment dictionary whose float payloads are fp16-representable, so fp32 and fp16 blobs hold the same numbers."""
    q = (lambda a: a.astype(np.float16).astype(np.float32)) if half_exact else (lambda a: a)
    poses = np.tile(np.eye(4, dtype=np.float32)[None, :3], (21, 1, 1))
    poses[:, :, 3] = rng.normal(0, 1, (21, 3))
    return {'poses': q(poses), 'model.density_bitfield': rng.integers(0, 256, dr.BITFIELD_BYTES, dtype=np.uint8),
            'model.hash_encoder.params': q(rng.uniform(-1, 1, dr.TOTAL_ENTRIES * 4).astype(np.float32)), 'model.per_level_scale': dr.LOG_B,
            'model.xyz_encoder.params': q(rng.normal(0, 1, 512).astype(np.float32)),
            'model.rgb_net.params': q(rng.normal(0, 1, 768).astype(np.float32))}


@pytest.fixture(scope="module")
def model_dict():
    return _model_dict(np.random.default_rng(77))


def test_npy_and_blob_folders_give_equal_arrays(hip_lib, model_dict, tmp_path):
    from ngp_hip.deploy import DeployedModel
    from ngp_hip.export import export_deployment_bins
    np.save(tmp_path / "deployment.npy", model_dict)
    a = DeployedModel.from_npy(str(tmp_path / "deployment.npy"))
    b = DeployedModel.from_npy(model_dict)
    export_deployment_bins(model_dict, tmp_path / "f32", dtype=np.float32)
    export_deployment_bins(str(tmp_path / "deployment.npy"), tmp_path / "f16", dtype=np.float16)
    c, d = DeployedModel.from_bins(tmp_path / "f32"), DeployedModel.from_bins(str(tmp_path / "f16"))
    assert os.path.getsize(tmp_path / "f16" / "hash_embedding.bin") == 8 + 2 * dr.TOTAL_ENTRIES * 4
    for m in (a, b, c, d):
        arr = m.arrays()
        assert arr["hash_table"].dtype == np.float32 and arr["density_bitfield"].dtype == np.uint8
        assert np.array_equal(arr["hash_table"], model_dict['model.hash_encoder.params'])
        assert np.array_equal(arr["sigma_weights"], model_dict['model.xyz_encoder.params'])
        assert np.array_equal(arr["rgb_weights"], model_dict['model.rgb_net.params'])
        assert np.array_equal(arr["density_bitfield"], model_dict['model.density_bitfield'])
    assert a.poses.shape == (21, 3, 4) and np.array_equal(c.poses[0], model_dict['poses'][20]) and np.array_equal(d.poses[0], c.poses[0])


def test_validation_errors(hip_lib, model_dict, tmp_path):
    from ngp_hip.deploy import DeployedModel
    from ngp_hip.export import export_deployment_bins, write_bin

    def bad(**kw):
        d = dict(model_dict)
        d.update(kw)
        return d

    t = model_dict['model.hash_encoder.params']
    for d, what in ((bad(**{'model.hash_encoder.params': t[:-4]}), "hash table"),
                    (bad(**{'model.per_level_scale': dr.LOG_B * (1 + 3e-6)}), "per_level_scale"),
                    (bad(**{'model.per_level_scale': 1.3195079565048218}), "per_level_scale"),           # b instead of ln b
                    (bad(**{'model.xyz_encoder.params': np.zeros(2048 + 1024, np.float32)}), "sigma weights"),
                    (bad(**{'model.rgb_net.params': np.zeros(767, np.float32)}), "rgb weights"),
                    (bad(**{'model.density_bitfield': np.zeros(2 * dr.BITFIELD_BYTES, np.uint8)}), "bitfield"),   # two cascades
                    (bad(**{'model.hash_encoder.params': t.astype(np.float64)}), "dtype")):
        with pytest.raises(ValueError, match=what):
            DeployedModel.from_npy(d)
    ok = DeployedModel.from_npy(bad(**{'model.per_level_scale': dr.LOG_B * (1 + 5e-7)}))              # inside the relative 1e-6
    assert ok.hash_table.size == t.size
    d = dict(model_dict); del d['model.rgb_net.params']
    with pytest.raises(ValueError, match="lacks model.rgb_net.params"):
        DeployedModel.from_npy(d)
    with pytest.raises(ValueError, match="no deployment model"):
        DeployedModel.from_npy(str(tmp_path / "missing.npy"))
    export_deployment_bins(model_dict, tmp_path / "b", dtype=np.float16)
    os.remove(tmp_path / "b" / "sigma_weights.bin")
    with pytest.raises(ValueError, match="lacks sigma_weights.bin"):
        DeployedModel.from_bins(tmp_path / "b")
    write_bin(str(tmp_path / "b" / "sigma_weights.bin"), np.zeros(512, np.int32))                       # a dtype code no payload uses
    with pytest.raises(ValueError, match="dtype"):
        DeployedModel.from_bins(tmp_path / "b")
    with open(tmp_path / "b" / "sigma_weights.bin", "wb") as f:                                         # a dtype code the format lacks
        f.write(np.array([9, 512], np.int32).tobytes() + np.zeros(512, np.float32).tobytes())
    with pytest.raises(ValueError, match="bad header"):
        DeployedModel.from_bins(tmp_path / "b")
    write_bin(str(tmp_path / "b" / "sigma_weights.bin"), np.zeros(512, np.float16))
    write_bin(str(tmp_path / "b" / "density_bitfield.bin"), np.zeros(dr.BITFIELD_BYTES // 4 - 1, np.uint32))
    with pytest.raises(ValueError, match="bitfield"):
        DeployedModel.from_bins(tmp_path / "b")
    with pytest.raises(ValueError, match="mode"):
        DeployedModel.from_npy(model_dict).render(np.eye(4)[:3], mode="fast")


def test_from_module_round_trip_and_refusal(hip_lib, tmp_path):
    """from_module takes train.py's deployment architecture only; what it extracts is what save_deployment_model writes."""
    import torch
    from modules.networks import NGP
    from modules.utils import save_deployment_model
    from ngp_hip.deploy import DEPLOYMENT_CONFIG, DeployedModel
    for kw in (dict(scale=0.5, max_res=1024), dict(DEPLOYMENT_CONFIG, rgb_net_width=32), dict(DEPLOYMENT_CONFIG, max_res=256),
               dict(DEPLOYMENT_CONFIG, scale=2.0), dict(DEPLOYMENT_CONFIG, rgb_net_depth=2)):
        with pytest.raises(ValueError, match="deployment architecture"):
            DeployedModel.from_module(NGP(**kw))
    torch.manual_seed(5)
    model = NGP(**DEPLOYMENT_CONFIG)
    model.density_bitfield.random_(0, 256)

    class Data:
        poses = torch.randn(24, 3, 4)

    save_deployment_model(model, Data, tmp_path)
    a, b = DeployedModel.from_module(model), DeployedModel.from_npy(str(tmp_path / "deployment.npy"))
    for k, v in a.arrays().items():
        assert np.array_equal(v, b.arrays()[k]), k
    assert np.array_equal(a.rgb_weights[512 + 48:], np.zeros(13 * 16, np.float32))                       # the zero padding of the colour rows
