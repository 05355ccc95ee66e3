"""The serial reference of the fused deployment render (tests/deploy_render_reference.py) on the CPU: its float32 restatement against
float64 gives the bounds the GPU tests use, the near-tie rule excludes few rays, early termination is exercised, and its image is the
reference program's on the rays that finished.  Plus the argument validation of the fused mode that needs no GPU."""
import numpy as np
import pytest

import deploy_reference as dr
import deploy_render_reference as rr


@pytest.fixture(scope="module")
def lib_scale(hip_lib):
    from ngp_hip import ops
    return ops.levels_to_numpy(ops.make_levels(2**21, 4, 32, 128, 4))[0]


@pytest.mark.parametrize("name,thr", sorted(rr.BOUNDS))
def test_bounds_are_four_times_the_restatement_distance(oracle, lego_bitfield, lib_scale, name, thr):
    """BOUNDS / 4 is the float32 restatement's distance from float64 on the non-tie rays, within 25 %; at most 1 % of the rays are near
    ties; float32 and float64 count the same samples on every other ray."""
    sc = rr.scene(name, oracle, lego_bitfield, lib_scale)
    dist, r64, r32, tie = rr.distances(sc, thr)
    print("%s T_threshold %g: %d rays, %d marched samples, %d composited, %d near ties; f32 vs f64 rgb %.3e opacity %.3e depth %.3e, bounds %s"
          % (name, thr, len(tie), sc.marched.sum(), r64[3].sum(), tie.sum(), dist[0], dist[1], dist[2], rr.BOUNDS[(name, thr)]))
    assert tie.mean() <= rr.TIE_SHARE
    assert np.array_equal(r64[3][~tie], r32[3][~tie]) and np.array_equal(r64[4][~tie], r32[4][~tie])
    for d, b in zip(dist, rr.BOUNDS[(name, thr)]):
        assert 0.75 * b / 4 <= d <= 1.25 * b / 4, (d, b)


def test_early_termination_is_exercised(oracle, lego_bitfield, lib_scale):
    """At T_threshold 0.3 more than half of the fixture image's rays that hold samples end by the threshold, in front of their last marched
    sample; at 1e-2 some do.  A miss has no samples and zero outputs."""
    sc = rr.scene("image", oracle, lego_bitfield, lib_scale)
    for thr, share in ((0.3, 0.5), (1e-2, 0.0)):
        rgb, op, dep, count, t_last, _ = sc.composite(thr)
        holds = sc.marched > 0
        ended = holds & (count < sc.marched)
        print("T_threshold %g: %d of %d rays with samples end by the threshold; %d of %d marched samples composited"
              % (thr, ended.sum(), holds.sum(), count.sum(), sc.marched.sum()))
        assert ended.sum() > share * holds.sum() and (count[holds] >= 1).all()
        none = ~holds
        assert none.sum() >= 1 and not rgb[none].any() and not op[none].any() and not dep[none].any() and not t_last[none].any()


def test_caps_take_a_prefix(oracle, lego_bitfield, lib_scale):
    """A cap of max_samples composites the first samples of the uncapped run: count = min(count, cap) and t_last is that sample's t."""
    sc = rr.scene("image", oracle, lego_bitfield, lib_scale)
    full = sc.composite(1e-2)[3]
    for cap in (1, 7, 64):
        _, _, _, count, t_last, _ = sc.composite(1e-2, cap)
        assert np.array_equal(count, np.minimum(full, cap))
        has = count > 0
        assert np.array_equal(t_last[has], sc.ts[sc.start[has] + count[has] - 1])


def test_restatement_image_is_the_progressive_fixture_where_it_finished(oracle, lego_bitfield):
    """The rule of test_oneshot_agrees_where_progressive_finished: every ray the reference's round budget did not run out on has the
    reference program's colour and opacity within 1e-3 (the reference's own level scales, as in test_restatement_image)."""
    fx = rr.fixture()
    w, h = (int(v) for v in fx["img_res_wh"])
    rgb, op, _, count, _, _ = rr.render_serial(oracle, (fx["pose"], dr.directions(w, h)), lego_bitfield,
                                               rr.table_of(float(fx["img_table_amplitude"])), rr.levels_for(fx["level_scale"]),
                                               fx["sigma_weights_syn"], fx["rgb_weights_syn"], float(fx["img_T_threshold"]), rr.MAX_SAMPLES,
                                               np.float32)
    finished = np.ones(w * h, bool)
    finished[fx["img_alive_at_end"]] = False
    ec, eo = np.abs(rgb - fx["img_rgb"])[finished].max(), np.abs(op - fx["img_opacity"])[finished].max()
    print("serial restatement vs the reference image on %d finished rays: rgb %.3e opacity %.3e" % (finished.sum(), ec, eo))
    assert finished.sum() == w * h - len(fx["img_alive_at_end"]) > w * h // 2 and count.sum() > 0
    assert ec <= 1e-3 and eo <= 1e-3


def test_ray_sets_cover_the_cases(oracle, lego_bitfield, lib_scale):
    sc = rr.scene("list", oracle, lego_bitfield, lib_scale)
    o, d = sc.rays_o, sc.rays_d
    miss, inside, zero = sc.hits[:, 0] < 0, (np.abs(o) < 0.5).all(1), (d == 0).any(1)
    assert miss.sum() >= 100 and inside.sum() >= 250 and zero.sum() >= 250 and (zero & miss).sum() >= 10 and (zero & ~miss).sum() >= 100
    assert (sc.marched[inside] > 0).sum() >= 100 and (sc.marched[zero] > 0).sum() >= 50 and sc.marched[0] > 0
    assert np.allclose(sc.hits[inside & ~miss, 0], 0.01)                                                      # the near plane
    ones = rr.scene("ones", oracle, lego_bitfield, lib_scale)
    assert ones.marched.max() == rr.MAX_SAMPLES and (ones.marched == rr.MAX_SAMPLES).sum() >= 10 and (ones.marched > 0).all()
    count = ones.composite(1e-2)[3]
    assert np.array_equal(count, ones.marched)                                                                # nothing ends by the threshold
    assert rr.scene("zeros", oracle, lego_bitfield, lib_scale).marched.sum() == 0


# ---------------------------------------------------------------------------------------------------- validation without a GPU
def test_mode_validation_names_all_three(hip_lib):
    from ngp_hip.deploy import DeployedModel
    rng = np.random.default_rng(5)
    m = DeployedModel(np.zeros(dr.TOTAL_ENTRIES * 4, np.float32), rng.normal(0, 1, 512).astype(np.float32),
                      rng.normal(0, 1, 768).astype(np.float32), np.zeros(dr.BITFIELD_BYTES, np.uint8))
    with pytest.raises(ValueError, match="'oneshot', 'progressive' or 'fused'"):
        m.render(np.eye(4)[:3], mode="fast")
    import inspect
    assert inspect.signature(m.render).parameters["mode"].default == "oneshot"


def test_deploy_render_argument_validation(hip_lib):
    """Shapes, dtypes, the level table, the cap and the table's alignment are refused with ValueError before anything is launched (host
    tensors: a call that passed them would end in the 'no CPU path' RuntimeError instead)."""
    import torch
    from ngp_hip import ops
    lv = ops.make_levels(2**21, 4, 32, 128, 4)
    good = dict(rays_o=torch.zeros(5, 3), rays_d=torch.ones(5, 3), density_bitfield=torch.zeros(dr.BITFIELD_BYTES, dtype=torch.uint8), coarse=None,
                table=torch.zeros(dr.TOTAL_ENTRIES * 4), lv=lv, sigma_w=torch.zeros(512), rgb_w=torch.zeros(768))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.deploy_render(**good)
    unaligned = torch.zeros(dr.TOTAL_ENTRIES * 4 + 1)[1:]
    assert unaligned.data_ptr() % 16 == 4
    for kw, what in ((dict(rays_d=torch.ones(4, 3)), "rays_d"), (dict(rays_o=torch.zeros(5, 3, dtype=torch.float64)), "rays_o"),
                     (dict(table=torch.zeros(16)), "hash_table"), (dict(sigma_w=torch.zeros(511)), "sigma_weights"),
                     (dict(rgb_w=torch.zeros(768, dtype=torch.float16)), "rgb_weights"),
                     (dict(density_bitfield=torch.zeros(2 * dr.BITFIELD_BYTES, dtype=torch.uint8)), "density_bitfield"),
                     (dict(density_bitfield=torch.zeros(dr.BITFIELD_BYTES, dtype=torch.int8)), "density_bitfield"),
                     (dict(coarse=torch.zeros(64, dtype=torch.int32)), "coarse"), (dict(lv=ops.make_levels(2**19, 16, 16, 1024, 2)), "level table"),
                     (dict(max_samples=0), "max_samples"), (dict(table=unaligned), "aligned"),
                     (dict(out=(torch.zeros(5, 3), torch.zeros(5), torch.zeros(5), torch.zeros(5), torch.zeros(5))), "n_samples")):
        with pytest.raises(ValueError, match=what):
            ops.deploy_render(**dict(good, **kw))
