"""Serial numpy reference of the fused deployment render (ngp_deploy_render, DeployedModel.render(mode="fused")), used by
tests/test_deploy_render.py and tests/test_gpu_deploy_fused.py.

Per ray: the CPU oracle's slab test and training march with zero noise (the sample sequence the kernel must reproduce bit for bit),
deploy_reference.shade on every marched sample, then the serial front-to-back composite of volume_train.py:34-48 -- before each sample
stop unless T > T_threshold; a = 1 - exp(-sigma dt), w = a T, rgb += w c, depth += w t, opacity += w, T *= 1 - a.  dtype=np.float64 is
the yardstick, dtype=np.float32 the restatement of the kernel's arithmetic (every operation a separate binary32 one); BOUNDS is four times
the distance between the two, the margin deploy_reference.BOUNDS uses for the shading alone (profiles/PARITY_NOTES.md).

The march and the shading do not depend on T_threshold, and a march capped at fewer samples is a prefix of the longer one, so a ray set
is marched and shaded once per dtype (`Scene`, cached per name) and composited per (threshold, cap)."""
import os

import numpy as np

import deploy_reference as dr

SCALE, CASCADES, GRID = 0.5, 1, 128
MAX_SAMPLES = 1024
TIE = 1e-4              # a ray with min_k |T_k / T_threshold - 1| below this may end one sample earlier or later in another arithmetic
TIE_SHARE = 0.01        # at most this share of a compared batch may be such rays

# 4 x the distance of the float32 restatement from the float64 one, (rgb, opacity, depth), rounded up to two digits, on the rays of the
# GPU tests: the 24x48 fixture image at both thresholds, the mixed ray list and the all-ones bitfield.  tests/test_deploy_render.py
# re-measures every row on the CPU (measured distances: 3.897e-6 3.529e-6 3.937e-6 / 3.897e-6 3.761e-6 5.911e-6 / 4.975e-6
# 5.099e-6 5.175e-6 / 1.210e-6 1.536e-6 4.539e-6); none comes from the kernel.
BOUNDS = {("image", 1e-2): (1.6e-5, 1.5e-5, 1.6e-5), ("image", 0.3): (1.6e-5, 1.6e-5, 2.4e-5), ("list", 1e-2): (2.0e-5, 2.1e-5, 2.1e-5),
          ("ones", 1e-2): (4.9e-6, 6.2e-6, 1.9e-5)}


def round_up_2(x):
    """x rounded up to two significant digits."""
    e = int(np.floor(np.log10(x))) - 1
    return float(np.ceil(x / 10.0**e - 1e-9) * 10.0**e)


class Scene:
    """One ray set marched once by the CPU oracle (zero noise, MAX_SAMPLES) and shaded once per dtype."""

    def __init__(self, ora, rays_o, rays_d, bitfield, table, levels, sigma_w, rgb_w):
        self.rays_o, self.rays_d = np.ascontiguousarray(rays_o, np.float32), np.ascontiguousarray(rays_d, np.float32)
        self.bitfield = np.ascontiguousarray(bitfield).reshape(-1).view(np.uint8)
        self.table, self.levels, self.sigma_w, self.rgb_w = table, levels, sigma_w, rgb_w
        n = self.rays_o.shape[0]
        self.hits = np.ascontiguousarray(ora.ray_aabb(self.rays_o, self.rays_d, SCALE))
        rays_a, self.xyzs, self.dirs, self.deltas, self.ts, _ = ora.march_train(
            self.rays_o, self.rays_d, self.hits, self.bitfield, np.zeros(n, np.float32), CASCADES, SCALE, 0.0, GRID, MAX_SAMPLES)
        assert np.array_equal(rays_a[:, 0], np.arange(n))                       # the serial march packs in ray order
        self.start, self.marched = rays_a[:, 1].astype(np.int64), rays_a[:, 2].astype(np.int64)
        self._shaded = {}

    def shaded(self, dtype):
        if dtype not in self._shaded:
            _, sigma, rgb = dr.shade(self.xyzs, self.dirs, self.table, self.levels, self.sigma_w, self.rgb_w, dtype)
            self._shaded[dtype] = (sigma, rgb)
        return self._shaded[dtype]

    def composite(self, T_threshold, max_samples=MAX_SAMPLES, dtype=np.float64):
        """-> rgb [n,3], opacity, depth (dtype), count (int64), t_last (f32, the oracle's sample), tie (f64)."""
        sigma, rgbs = self.shaded(dtype)
        n = self.rays_o.shape[0]
        thr = dtype(np.float32(T_threshold))
        limit = np.minimum(self.marched, int(max_samples))
        rgb, op, dep = np.zeros((n, 3), dtype), np.zeros(n, dtype), np.zeros(n, dtype)
        T = np.ones(n, dtype)
        count, t_last, tie = np.zeros(n, np.int64), np.zeros(n, np.float32), np.full(n, np.inf)
        for j in range(int(limit.max()) if n else 0):
            r = np.flatnonzero((j < limit) & (count == j) & (T > thr))       # rays that composite their sample j
            if r.size == 0:
                break
            s = self.start[r] + j
            a = dtype(1.0) - np.exp(-sigma[s] * self.deltas[s].astype(dtype))
            w = a * T[r]
            rgb[r] = rgb[r] + w[:, None] * rgbs[s]
            dep[r] = dep[r] + w * self.ts[s].astype(dtype)
            op[r] = op[r] + w
            T[r] = T[r] * (dtype(1.0) - a)
            count[r] += 1
            t_last[r] = self.ts[s]
            if thr > 0:
                tie[r] = np.minimum(tie[r], np.abs(T[r].astype(np.float64) / np.float64(thr) - 1.0))
        return rgb, op, dep, count, t_last, tie


def render_serial(ora, pose_or_rays, bitfield, table, levels, sigma_w, rgb_w, T_threshold, max_samples=MAX_SAMPLES, dtype=np.float64):
    """pose_or_rays: (pose 3x4, camera-frame directions [n,3]) or (rays_o [n,3], rays_d [n,3]).
    -> rgb, opacity, depth, per-ray count, per-ray t_last, per-ray tie = min_k |T_k / T_threshold - 1| over the composited prefix."""
    a, b = pose_or_rays
    if np.asarray(a).size == 12:
        a, b = ora.get_rays(np.asarray(b, np.float32), np.asarray(a, np.float32).reshape(3, 4))
    return Scene(ora, a, b, bitfield, table, levels, sigma_w, rgb_w).composite(T_threshold, max_samples, dtype)


# ---------------------------------------------------------------------------------------------------- the ray sets of the tests
def fixture():
    from conftest import GOLDEN
    return dict(np.load(os.path.join(GOLDEN, "ref_deploy.npz")))


def levels_for(lib_scale=None):
    """The level table; the scales are the library's own where given (ops.levels_to_numpy(lv)[0]), else numpy's f32 exp."""
    scale, res, size, offset = dr.level_table()
    return (scale if lib_scale is None else np.asarray(lib_scale, np.float32)), res, size, offset


def ray_list(n=1153, seed=19):
    """A seeded list that cycles through four kinds: a camera ray into the box from outside, a ray that misses it, a ray that starts
    inside it, and a ray with one or two zero direction components (every fourth of those misses as well)."""
    rng = np.random.default_rng(seed)
    o, d = np.empty((n, 3), np.float32), np.empty((n, 3), np.float32)
    for i in range(n):
        kind = i % 4
        target = rng.uniform(-0.2, 0.2, 3)                                   # the trained scene sits in the middle of the box
        if kind == 0:
            p = rng.normal(0, 1, 3); p = 1.6 * p / np.linalg.norm(p)
            v = (target - p) / np.linalg.norm(target - p) * rng.uniform(0.7, 1.4)
        elif kind == 1:
            p = rng.normal(0, 1, 3); p = 1.6 * p / np.linalg.norm(p)
            v = -(target - p) / np.linalg.norm(target - p) if i % 8 == 1 else np.cross(p, rng.normal(0, 1, 3))
            v = v / np.linalg.norm(v)
        elif kind == 2:
            p = rng.uniform(-0.45, 0.45, 3)
            v = (target - p) / np.linalg.norm(target - p)
        else:
            ax = int(rng.integers(0, 3))
            v = rng.normal(0, 1, 3); v[ax] = 0.0
            if i % 8 == 3:
                v[(ax + 1) % 3] = 0.0
            v = v / np.linalg.norm(v)
            p = target - 1.3 * v
            if i % 16 == 7:
                p[ax] = 0.75                                                     # parallel to a slab and outside it: a miss
        o[i], d[i] = p, v
    return o, d


def ones_rays(n=256, seed=23):
    """Rays through the box for the all-ones bitfield: directions of length 0.3 .. 1.5, so the longest hold more orbit points than the
    cap; the first two run along a diagonal of the box."""
    rng = np.random.default_rng(seed)
    p = rng.normal(0, 1, (n, 3)); p = 1.5 * p / np.linalg.norm(p, axis=1, keepdims=True)
    target = rng.uniform(-0.3, 0.3, (n, 3))
    v = target - p
    v = v / np.linalg.norm(v, axis=1, keepdims=True) * rng.uniform(0.3, 1.5, (n, 1))
    p[0], v[0] = (-1.0, -1.0, -1.0), (0.5, 0.5, 0.5)
    p[1], v[1] = (1.0, -1.0, 1.0), (-0.25, 0.25, -0.25)
    return p.astype(np.float32), v.astype(np.float32)


ONES_TABLE_AMPLITUDE = 0.05     # a thin medium: sigma ~ 1, so no ray of the all-ones case ends by T_threshold 1e-2 before the cap or the box
_scenes = {}


def scene(name, ora, lego_bitfield, lib_scale=None):
    """The cached Scene of a test ray set: "image" (the 24x48 fixture image), "list" (ray_list), "ones" (all-ones bitfield), "zeros"."""
    key = (name, None if lib_scale is None else tuple(np.asarray(lib_scale, np.float32).view(np.uint32).tolist()))
    if key not in _scenes:
        fx = fixture()
        lv = levels_for(lib_scale)
        sw, rw = fx["sigma_weights_syn"], fx["rgb_weights_syn"]
        if name == "image":
            w, h = (int(v) for v in fx["img_res_wh"])
            o, d = ora.get_rays(dr.directions(w, h), fx["pose"].astype(np.float32).reshape(3, 4))
            args = (o, d, lego_bitfield, table_of(float(fx["img_table_amplitude"])))
        elif name == "list":
            args = ray_list() + (lego_bitfield, table_of(float(fx["img_table_amplitude"])))
        elif name == "ones":
            args = ones_rays() + (np.full(dr.BITFIELD_BYTES, 255, np.uint8), table_of(ONES_TABLE_AMPLITUDE))
        elif name == "zeros":
            args = ones_rays() + (np.zeros(dr.BITFIELD_BYTES, np.uint8), table_of(ONES_TABLE_AMPLITUDE))
        else:
            raise KeyError(name)
        _scenes[key] = Scene(ora, *args, lv, sw, rw)
    return _scenes[key]


_tables = {}


def table_of(amplitude):
    if amplitude not in _tables:
        _tables[amplitude] = dr.synthetic_table(amplitude)
    return _tables[amplitude]


def distances(sc, T_threshold, max_samples=MAX_SAMPLES):
    """The float32 restatement against float64 on the non-tie rays of a scene: (rgb, opacity, depth) max abs distance, the float64 and
    float32 results and the tie mask."""
    r64 = sc.composite(T_threshold, max_samples, np.float64)
    r32 = sc.composite(T_threshold, max_samples, np.float32)
    tie = r64[5] < TIE
    keep = ~tie
    dist = tuple(float(np.abs(r32[k][keep].astype(np.float64) - r64[k][keep]).max()) for k in range(3))
    return dist, r64, r32, tie
