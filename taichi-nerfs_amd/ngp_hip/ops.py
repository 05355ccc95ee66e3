"""Tensor-level launchers over the C ABI: allocate outputs with torch, pass raw device pointers + the current
torch HIP stream.  No autograd here (that lives in modules/), no CPU path: every function requires device
tensors and raises otherwise."""
import ctypes
import os
from types import SimpleNamespace

import numpy as np
import torch

from . import lib as _lib_mod
from .lib import HashLevels, TriPlaneLevels, check


def _lib():
    return _lib_mod.load()


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream():
    """torch's current HIP stream on the current device as a void* (every launch goes there).  torch.cuda.current_stream() builds
    a Stream object per call (~10 us, nine calls per training step of the operator path: profiles/r04_train_py_cprofile.txt);
    the raw getter is the same handle without the object."""
    if _raw_stream is not None:
        return ctypes.c_void_p(_raw_stream(torch.cuda.current_device()))
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _touched(*tensors):
    """A kernel wrote these tensors IN PLACE through their raw pointers: move their torch version counters like any in-place
    torch op would, so version-keyed caches (the trainer's coarse occupancy table) and autograd's saved-tensor checks see it."""
    for t in tensors:
        if t is not None:
            torch.autograd.graph.increment_version(t)


def _dev(t, dtype=None, name="tensor"):
    if not t.is_cuda:
        raise RuntimeError("%s must live on the GPU: libngp_hip has no CPU path (got device %s)" % (name, t.device))
    if dtype is not None and t.dtype != dtype:
        raise TypeError("%s must be %s, got %s" % (name, dtype, t.dtype))
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous" % name)
    return t


def make_levels(max_params, levels, base_res, max_res, features):
    """ngp_hash_levels table (host struct) -- HashEncoder.__init__ arithmetic (hash_encoder.py:183-205)."""
    lv = HashLevels()
    check(_lib().ngp_hash_levels_init(ctypes.byref(lv), float(max_params), int(levels), float(base_res), float(max_res),
                                      int(features)), "ngp_hash_levels_init")
    return lv


# ---------------------------------------------------------------------------------------------------- a-1
def ray_aabb(rays_o, rays_d, scale):
    _dev(rays_o, torch.float32, "rays_o"); _dev(rays_d, torch.float32, "rays_d")
    n = rays_o.shape[0]
    hits_t = torch.empty(n, 2, device=rays_o.device, dtype=torch.float32)
    check(_lib().ngp_ray_aabb(_ptr(rays_o), _ptr(rays_d), float(scale), n, _ptr(hits_t), _stream()), "ngp_ray_aabb")
    return hits_t


# ---------------------------------------------------------------------------------------------------- a-2
class MarchArena:
    """Per-device staging rows for the training march: [n_rays * max_samples] (t, dt) pairs.

    Worst case like the reference's N*1024 torch.empty buffers (ray_march.py:144-168) but allocated once and
    reused; only the rows/entries actually emitted are ever touched (288 GB of HBM makes the reservation free)."""
    _cache = {}

    @classmethod
    def get(cls, device, n_rays, max_samples):
        key = (device.index if device.index is not None else torch.cuda.current_device())
        need = n_rays * max_samples
        cur = cls._cache.get(key)
        if cur is None or cur.shape[0] < need:
            cur = torch.empty(need, 2, device=device, dtype=torch.float32)
            cls._cache[key] = cur
        return cur


def coarse_bitfield(density_bitfield, cascades, grid_size, out=None):
    """One bit per 8^3-cell block (any cell occupied) -- the shortcut table of ngp_march_train_count_ex."""
    words = int(cascades) * int(grid_size)**3 // 512 // 32
    if out is None:
        out = torch.empty(words, device=density_bitfield.device, dtype=torch.int32)
    check(_lib().ngp_bitfield_coarsen(_ptr(density_bitfield), int(cascades), int(grid_size), _ptr(out), _stream()),
          "ngp_bitfield_coarsen")
    return out


def march_train(rays_o, rays_d, hits_t, density_bitfield, noise, cascades, scale, exp_step_factor, grid_size, max_samples):
    """count -> scan -> (one D2H read of the total, like ray_march.py:187-192) -> write."""
    _dev(rays_o, torch.float32, "rays_o"); _dev(rays_d, torch.float32, "rays_d"); _dev(hits_t, torch.float32, "hits_t")
    _dev(density_bitfield, torch.uint8, "density_bitfield"); _dev(noise, torch.float32, "noise")
    n = rays_o.shape[0]
    dev = rays_o.device
    L = _lib()
    stage = MarchArena.get(dev, n, int(max_samples))
    counts = torch.empty(n, device=dev, dtype=torch.int32)
    rays_a = torch.empty(n, 3, device=dev, dtype=torch.int32)
    total = torch.zeros(1, device=dev, dtype=torch.int32)
    st = _stream()
    coarse = coarse_bitfield(density_bitfield, cascades, grid_size)
    check(L.ngp_march_train_count_ex(_ptr(rays_o), _ptr(rays_d), _ptr(hits_t), _ptr(density_bitfield), _ptr(coarse), _ptr(noise),
                                     int(cascades), int(grid_size), float(scale), float(exp_step_factor), int(max_samples), n,
                                     _ptr(stage), _ptr(counts), st), "ngp_march_train_count_ex")
    check(L.ngp_march_train_scan(_ptr(counts), n, _ptr(rays_a), _ptr(total), st), "ngp_march_train_scan")
    S = int(total.item())
    xyzs = torch.empty(S, 3, device=dev, dtype=torch.float32)
    dirs = torch.empty(S, 3, device=dev, dtype=torch.float32)
    deltas = torch.empty(S, device=dev, dtype=torch.float32)
    ts = torch.empty(S, device=dev, dtype=torch.float32)
    if S > 0:
        check(L.ngp_march_train_write(_ptr(rays_o), _ptr(rays_d), _ptr(rays_a), _ptr(stage), int(max_samples), n,
                                      _ptr(xyzs), _ptr(dirs), _ptr(deltas), _ptr(ts), st), "ngp_march_train_write")
    return rays_a, xyzs, dirs, deltas, ts, total[0]


def march_train_fused(rays_o, rays_d, hits_t, density_bitfield, noise, cascades, scale, exp_step_factor, grid_size, max_samples,
                      capacity=None, seed=None, shape=None):
    """ngp_march_train_fused: the same samples per ray as march_train() in ONE launch, the rays packed in block-completion order
    (rays_a[r] = (r, start, count)); outputs are sized for `capacity` samples (default n * max_samples), the first `total` valid --
    with a smaller capacity the kernel drops what does not fit (compare the returned total with it).  hits_t may be None (slab
    test inline).  noise=None + seed: the jitter is drawn in the kernel, ray r gets rng_uniform(seed, r).  shape = (waves per
    block in {4, 8, 16}, bytes of idle dynamic LDS per block): ngp_march_train_fused_shaped (full-capacity outputs only)."""
    _dev(rays_o, torch.float32, "rays_o"); _dev(rays_d, torch.float32, "rays_d")
    _dev(density_bitfield, torch.uint8, "density_bitfield")
    if noise is None:
        if seed is None:
            raise ValueError("march_train_fused needs a noise vector or a seed")
    else:
        _dev(noise, torch.float32, "noise")
    n = rays_o.shape[0]
    dev = rays_o.device
    cap = n * int(max_samples) if capacity is None else int(capacity)
    if (shape is not None or noise is None) and cap < n * int(max_samples):
        raise ValueError("the %s form writes into arrays of n * max_samples rows" % ("shaped" if shape is not None else "seeded"))
    f32 = dict(device=dev, dtype=torch.float32)
    M = SimpleNamespace(stage=MarchArena.get(dev, n, int(max_samples)), rays_a=torch.empty(n, 3, device=dev, dtype=torch.int32),
                        total=torch.zeros(1, device=dev, dtype=torch.int32), ctr=torch.zeros(2, device=dev, dtype=torch.int32),
                        xyzs=torch.empty(cap, 3, **f32), dirs=torch.empty(cap, 3, **f32), deltas=torch.empty(cap, **f32),
                        ts=torch.empty(cap, **f32))
    coarse = coarse_bitfield(density_bitfield, cascades, grid_size)
    launch_march_train(_lib(), M, rays_o, rays_d, hits_t, density_bitfield, coarse, noise, seed or 0, cascades, grid_size, scale,
                       exp_step_factor, max_samples, shape=shape, cap=cap)
    return M.rays_a, M.xyzs, M.dirs, M.deltas, M.ts, M.total[0], M.ctr


def launch_march_train(L, M, rays_o, rays_d, hits_t, bitfield, coarse, noise, seed, cascades, grid_size, scale, exp_step_factor,
                       max_samples, shape=None, cap=None, ray_order=False):
    """The training march into buffers the caller owns (M.stage, .ctr, .rays_a, .total, .xyzs, .dirs, .deltas, .ts; .counts for
    ray_order), on the current stream -- the one place that picks the ngp_march_train_* entry:
      ray_order      the count / scan / write chain (rays packed in ray order; needs a noise vector);
      shape          ngp_march_train_fused_shaped (waves per block, idle LDS bytes; jitter from `noise`, else from `seed`);
      noise is None  ngp_march_train_fused_rng: the jitter drawn in the kernel from `seed`;
      otherwise      ngp_march_train_fused on `noise`, or _fused_cap when the outputs hold `cap` rows only."""
    n, st = rays_o.shape[0], _stream()
    rays = (_ptr(rays_o), _ptr(rays_d), _ptr(hits_t), _ptr(bitfield), _ptr(coarse))
    geom = (int(cascades), int(grid_size), float(scale), float(exp_step_factor), int(max_samples), n)
    out = (_ptr(M.stage), _ptr(M.ctr), _ptr(M.rays_a), _ptr(M.total), _ptr(M.xyzs), _ptr(M.dirs), _ptr(M.deltas), _ptr(M.ts), st)
    if ray_order:
        check(L.ngp_march_train_count_ex(*rays, _ptr(noise), *geom, _ptr(M.stage), _ptr(M.counts), st), "ngp_march_train_count_ex")
        check(L.ngp_march_train_scan(_ptr(M.counts), n, _ptr(M.rays_a), _ptr(M.total), st), "ngp_march_train_scan")
        check(L.ngp_march_train_write(_ptr(rays_o), _ptr(rays_d), _ptr(M.rays_a), _ptr(M.stage), int(max_samples), n,
                                      _ptr(M.xyzs), _ptr(M.dirs), _ptr(M.deltas), _ptr(M.ts), st), "ngp_march_train_write")
    elif shape is not None:
        check(L.ngp_march_train_fused_shaped(*rays, _ptr(noise), int(seed), *geom, int(shape[0]), int(shape[1]), *out),
              "ngp_march_train_fused_shaped")
    elif noise is None:
        check(L.ngp_march_train_fused_rng(*rays, int(seed), *geom, *out), "ngp_march_train_fused_rng")
    elif cap is None:
        check(L.ngp_march_train_fused(*rays, _ptr(noise), *geom, *out), "ngp_march_train_fused")
    else:
        check(L.ngp_march_train_fused_cap(*rays, _ptr(noise), *geom, int(cap), *out), "ngp_march_train_fused_cap")


def rng_uniform(seed, n, device="cuda"):
    """[n] float32: rng_uniform(seed, i) -- the jitter ngp_march_train_fused_rng(seed) gives ray i."""
    out = torch.empty(n, device=device, dtype=torch.float32)
    check(_lib().ngp_rng_uniform(int(seed), int(n), _ptr(out), _stream()), "ngp_rng_uniform")
    return out


def march_train_bwd(d_xyzs, d_dirs, ts, rays_a):
    """ngp_march_train_bwd: adjoint of xyzs = o + t d, dirs = d over the rows (ray_idx, start, N) of rays_a, t held constant.
    d_xyzs, d_dirs: [S,3] float32 or None (= zeros); ts [S]; rays_a [n,3] of march_train / march_train_fused, whose rows must
    address samples inside [0, S).  -> (d_rays_o, d_rays_d) [n,3], every row written, indexed by ray_idx."""
    _dev(ts, torch.float32, "ts"); _dev(rays_a, torch.int32, "rays_a")
    for name, t in (("d_xyzs", d_xyzs), ("d_dirs", d_dirs)):
        if t is not None:
            _dev(t, torch.float32, name)
            if t.ndim != 2 or t.shape[1] != 3 or t.shape[0] != ts.shape[0]:
                raise ValueError("%s must be [S,3] with S = len(ts) = %d, got %s" % (name, ts.shape[0], tuple(t.shape)))
    n = rays_a.shape[0]
    d_rays_o = torch.empty(n, 3, device=rays_a.device, dtype=torch.float32)
    d_rays_d = torch.empty(n, 3, device=rays_a.device, dtype=torch.float32)
    check(_lib().ngp_march_train_bwd(_ptr(d_xyzs), _ptr(d_dirs), _ptr(ts), _ptr(rays_a), n, _ptr(d_rays_o), _ptr(d_rays_d),
                                     _stream()), "ngp_march_train_bwd")
    return d_rays_o, d_rays_d


def sample_rays_bwd(directions, img_idx, img0, pix_idx, d_rays_o, d_rays_d, n_img):
    """ngp_sample_rays_bwd: d_poses [n_img,3,4] of the rays of ngp_sample_rays (or of get_rays with one pose: img_idx = None,
    img0 = 0, pix_idx = None, n_img = 1).  img_idx / pix_idx: [n] int64 or None (every ray from image img0 / pixel k of ray k);
    d_rays_o / d_rays_d: [n,3] float32 or None (= zeros), at least one given.  pix_idx must address rows of directions."""
    _dev(directions, torch.float32, "directions")
    grads = [g for g in (d_rays_o, d_rays_d) if g is not None]
    if not grads:
        raise ValueError("sample_rays_bwd needs d_rays_o or d_rays_d")
    n = grads[0].shape[0]
    for name, t in (("d_rays_o", d_rays_o), ("d_rays_d", d_rays_d)):
        if t is not None:
            _dev(t, torch.float32, name)
            if tuple(t.shape) != (n, 3):
                raise ValueError("%s must be [%d,3], got %s" % (name, n, tuple(t.shape)))
    for name, t in (("img_idx", img_idx), ("pix_idx", pix_idx)):
        if t is not None:
            _dev(t, torch.int64, name)
            if tuple(t.shape) != (n,):
                raise ValueError("%s must be [%d], got %s" % (name, n, tuple(t.shape)))
    if pix_idx is None and directions.shape[0] < n:
        raise ValueError("without pix_idx ray k reads directions[k]: %d directions for %d rays" % (directions.shape[0], n))
    d_poses = torch.empty(int(n_img), 3, 4, device=directions.device, dtype=torch.float32)
    check(_lib().ngp_sample_rays_bwd(_ptr(directions), _ptr(img_idx), ctypes.c_longlong(int(img0)), _ptr(pix_idx), _ptr(d_rays_o),
                                     _ptr(d_rays_d), n, int(n_img), _ptr(d_poses), _stream()), "ngp_sample_rays_bwd")
    return d_poses


def get_rays_bwd(directions, d_rays_o, d_rays_d):
    """ngp_get_rays_bwd: d_poses [n,3,4] of get_rays with one pose per ray; d_rays_o / d_rays_d [n,3] float32 or None (= zeros)."""
    _dev(directions, torch.float32, "directions")
    n = directions.shape[0]
    for name, t in (("d_rays_o", d_rays_o), ("d_rays_d", d_rays_d)):
        if t is not None:
            _dev(t, torch.float32, name)
            if tuple(t.shape) != (n, 3):
                raise ValueError("%s must be [%d,3], got %s" % (name, n, tuple(t.shape)))
    d_poses = torch.empty(n, 3, 4, device=directions.device, dtype=torch.float32)
    check(_lib().ngp_get_rays_bwd(_ptr(directions), _ptr(d_rays_o), _ptr(d_rays_d), n, _ptr(d_poses), _stream()), "ngp_get_rays_bwd")
    return d_poses


# ---------------------------------------------------------------------------------------------------- a-3
def march_test(rays_o, rays_d, hits_t, alive_indices, density_bitfield, cascades, scale, exp_step_factor, grid_size,
               max_samples):
    _dev(rays_o, torch.float32, "rays_o"); _dev(rays_d, torch.float32, "rays_d"); _dev(hits_t, torch.float32, "hits_t")
    _dev(alive_indices, torch.int64, "alive_indices"); _dev(density_bitfield, torch.uint8, "density_bitfield")
    n = alive_indices.shape[0]
    dev = rays_o.device
    ray_indices = torch.empty(n * max_samples, device=dev, dtype=torch.int64)
    valid_mask = torch.zeros(n * max_samples, device=dev, dtype=torch.uint8)
    deltas = torch.empty(n * max_samples, device=dev, dtype=torch.float32)
    ts = torch.empty(n * max_samples, device=dev, dtype=torch.float32)
    samples_counter = torch.empty(n, device=dev, dtype=torch.int32)
    check(_lib().ngp_march_test(_ptr(rays_o), _ptr(rays_d), _ptr(hits_t), _ptr(alive_indices), _ptr(density_bitfield),
                                int(cascades), int(grid_size), float(scale), float(exp_step_factor), int(max_samples), n,
                                _ptr(ray_indices), _ptr(valid_mask), _ptr(deltas), _ptr(ts), _ptr(samples_counter), _stream()),
          "ngp_march_test")
    _touched(hits_t)                                                  # resume state, advanced in place (ray_march.py:262-268)
    return ray_indices, valid_mask, deltas, ts, samples_counter


# ---------------------------------------------------------------------------------------------------- a-4/5
def hash_fwd_f32(xyzs, table, lv):
    _dev(xyzs, torch.float32, "xyzs"); _dev(table, torch.float32, "hash_table")
    n = xyzs.shape[0]
    out = torch.empty(n, lv.n_levels * lv.n_features, device=xyzs.device, dtype=torch.float32)
    check(_lib().ngp_hash_fwd_f32(_ptr(xyzs), _ptr(table), ctypes.byref(lv), n, _ptr(out), _stream()), "ngp_hash_fwd_f32")
    return out


def cast_bf16(src, dst=None):
    """dst = bf16(src), round-to-nearest-even (ngp_cast_f32_bf16); numel % 4 == 0."""
    _dev(src, torch.float32, "src")
    if dst is None:
        dst = torch.empty(src.shape, device=src.device, dtype=torch.bfloat16)
    _dev(dst, torch.bfloat16, "dst")
    check(_lib().ngp_cast_f32_bf16(_ptr(src), _ptr(dst), src.numel(), _stream()), "ngp_cast_f32_bf16")
    return dst


def hash_fwd_bf16(xyzs, table_bf16, lv):
    """bf16-stored table (F = 2), f32 interpolation and output [n, L*2]."""
    _dev(xyzs, torch.float32, "xyzs"); _dev(table_bf16, torch.bfloat16, "hash_table(bf16)")
    n = xyzs.shape[0]
    out = torch.empty(n, lv.n_levels * lv.n_features, device=xyzs.device, dtype=torch.float32)
    check(_lib().ngp_hash_fwd_bf16_ex(_ptr(xyzs), _ptr(table_bf16), ctypes.byref(lv), n, _ptr(None), 0, 0.0, 1.0, 0, _ptr(out),
                                      _stream()), "ngp_hash_fwd_bf16_ex")
    return out


SLICED_MIN_SAMPLES = 65536      # below this the float-atomic kernel wins (the sliced launch has a ~60 us floor: 1 k slice owners)


def hash_bwd_f32(xyzs, dout, lv, dtable):
    """dtable += scatter-add of dout (hash_encoder.py:269, the Taichi-autodiff backward).  Large batches take the LDS-sliced
    formulation (no global float atomics, f64 accumulation; 3x faster at training batch sizes), small ones -- or level tables
    it cannot express (F != 2, a level of more than 64 slices) -- the float-atomic kernel.  NGP_HASH_BWD=atomic forces the latter."""
    _dev(xyzs, torch.float32, "xyzs"); _dev(dout, torch.float32, "dout"); _dev(dtable, torch.float32, "dtable")
    n = xyzs.shape[0]
    if n >= SLICED_MIN_SAMPLES and os.environ.get("NGP_HASH_BWD", "sliced") != "atomic" and lv.n_features == 2:
        ws = sliced_workspace(lv, n, xyzs.device)
        rc = _lib().ngp_hash_bwd_f32_sliced(_ptr(xyzs), _ptr(dout), ctypes.byref(lv), n, _ptr(None), _ptr(None), 0, 0.0, 1.0, 0,
                                            _ptr(dtable), _ptr(None), _ptr(ws), ws.numel(), _stream())
        if rc != -2:
            check(rc, "ngp_hash_bwd_f32_sliced")
            _touched(dtable)
            return dtable
    check(_lib().ngp_hash_bwd_f32(_ptr(xyzs), _ptr(dout), ctypes.byref(lv), n, _ptr(dtable), _stream()),
          "ngp_hash_bwd_f32")
    _touched(dtable)
    return dtable


_sliced_ws = {}


def sliced_workspace(lv, n_max, device):
    """Scratch of the LDS-sliced scatter-add for buffers of n_max samples: one per (device, stream) -- the prepass's bitmaps and the
    persistent workgroups' queue heads live in it, so two backward passes in flight on different streams must not share one
    (on one stream the launches serialise and the buffer is reused).  Grown, never shrunk; a buffer that is replaced is
    handed back to torch's caching allocator, which keeps it away from other streams until this stream's pending work is done."""
    need = int(_lib().ngp_hash_bwd_sliced_workspace(ctypes.byref(lv), int(n_max)))
    dev_index = device.index if device.index is not None else torch.cuda.current_device()
    key = (dev_index, torch.cuda.current_stream(device).cuda_stream)
    ws = _sliced_ws.get(key)
    if ws is None or ws.numel() < need:
        ws = _sliced_ws[key] = torch.empty(need, device=device, dtype=torch.uint8)
    return ws


def hash_bwd_f32_sliced(xyzs, dout, lv, dtable, live_idx=None, n_dev=None):
    """dtable += scatter-add of dout (natural [n, L*2] layout), LDS-sliced formulation; xyzs in [0,1].  Raises if the level table
    does not fit (use hash_bwd_f32 then)."""
    _dev(xyzs, torch.float32, "xyzs"); _dev(dout, torch.float32, "dout"); _dev(dtable, torch.float32, "dtable")
    n = dout.shape[0]
    ws = sliced_workspace(lv, n, xyzs.device)
    check(_lib().ngp_hash_bwd_f32_sliced(_ptr(xyzs), _ptr(dout), ctypes.byref(lv), n, _ptr(n_dev), _ptr(live_idx), 0, 0.0, 1.0, 0,
                                         _ptr(dtable), _ptr(None), _ptr(ws), ws.numel(), _stream()), "ngp_hash_bwd_f32_sliced")
    _touched(dtable)
    return dtable


def hash_fwd_f16(xyzs, table_h, lv):
    _dev(xyzs, torch.float32, "xyzs"); _dev(table_h, torch.float16, "hash_table(f16)")
    n = xyzs.shape[0]
    out = torch.empty(n, lv.n_levels, lv.n_features, device=xyzs.device, dtype=torch.float16)
    check(_lib().ngp_hash_fwd_f16(_ptr(xyzs), _ptr(table_h), ctypes.byref(lv), n, _ptr(out), _stream()), "ngp_hash_fwd_f16")
    return out


def hash_bwd_f16(xyzs, dout_h, lv, dtable_h):
    """The half2 encoder's scatter-add (hash_encoder_half.py:163-213).  Like hash_bwd_f32: large batches take the LDS-sliced
    form (exact sum of the fp16 contributions, rounded once), small ones / unsupported tables the packed-f16-atomic kernel."""
    _dev(xyzs, torch.float32, "xyzs"); _dev(dout_h, torch.float16, "dout"); _dev(dtable_h, torch.float16, "dtable")
    n = xyzs.shape[0]
    if n >= SLICED_MIN_SAMPLES and os.environ.get("NGP_HASH_BWD", "sliced") != "atomic" and lv.n_features == 2:
        ws = sliced_workspace(lv, n, xyzs.device)
        L = _lib()
        rc = L.ngp_hash_bwd_sliced_prep(_ptr(xyzs), ctypes.byref(lv), n, _ptr(None), _ptr(None), 0, 0.0, 1.0, _ptr(ws), ws.numel(), _stream())
        if rc != -2:
            check(rc, "ngp_hash_bwd_sliced_prep")
            dout = dout_h.float().reshape(n, -1).contiguous()          # fp16 -> fp32 is exact; the kernel rounds back (a no-op)
            check(L.ngp_hash_bwd_sliced_main_f16(_ptr(dout), ctypes.byref(lv), n, _ptr(None), 0, _ptr(dtable_h), _ptr(None), _ptr(ws),
                                                 ws.numel(), _stream()), "ngp_hash_bwd_sliced_main_f16")
            _touched(dtable_h)
            return dtable_h
    check(_lib().ngp_hash_bwd_f16(_ptr(xyzs), _ptr(dout_h), ctypes.byref(lv), xyzs.shape[0], _ptr(dtable_h), _stream()),
          "ngp_hash_bwd_f16")
    _touched(dtable_h)
    return dtable_h


def hash_bwd_f16_sliced(xyzs, dout, lv, dtable_h, live_idx=None, n_dev=None):
    """dtable_h (fp16 [entries, 2]) += the half2 encoder's scatter-add of dout (fp32 [n, L*2], rounded to fp16 like the encoder's
    output gradient) in the LDS-sliced formulation: prepass + ngp_hash_bwd_sliced_main_f16; xyzs in [0,1]."""
    _dev(xyzs, torch.float32, "xyzs"); _dev(dout, torch.float32, "dout"); _dev(dtable_h, torch.float16, "dtable")
    n = dout.shape[0]
    ws = sliced_workspace(lv, n, xyzs.device)
    L = _lib()
    check(L.ngp_hash_bwd_sliced_prep(_ptr(xyzs), ctypes.byref(lv), n, _ptr(n_dev), _ptr(live_idx), 0, 0.0, 1.0, _ptr(ws), ws.numel(),
                                     _stream()), "ngp_hash_bwd_sliced_prep")
    check(L.ngp_hash_bwd_sliced_main_f16(_ptr(dout), ctypes.byref(lv), n, _ptr(n_dev), 0, _ptr(dtable_h), _ptr(None), _ptr(ws), ws.numel(),
                                         _stream()), "ngp_hash_bwd_sliced_main_f16")
    _touched(dtable_h)
    return dtable_h


# ---------------------------------------------------------------------------------------------------- a-4x
def _hash_bwd_input(entry, xyzs, table, table_dtype, denc, denc_dtype, lv):
    _dev(xyzs, torch.float32, "xyzs"); _dev(table, table_dtype, "hash_table"); _dev(denc, denc_dtype, "denc")
    n = xyzs.shape[0]
    if xyzs.numel() != 3 * n:
        raise ValueError("xyzs must be [n, 3], got %s" % (tuple(xyzs.shape),))
    if table.numel() != lv.total_entries * lv.n_features:
        raise ValueError("hash_table has %d elements, the level table describes %d" % (table.numel(), lv.total_entries * lv.n_features))
    if denc.numel() != n * lv.n_levels * lv.n_features:
        raise ValueError("denc must hold [n, levels * features] = %d x %d values, got %s"
                         % (n, lv.n_levels * lv.n_features, tuple(denc.shape)))
    dxyzs = torch.empty(n, 3, device=xyzs.device, dtype=torch.float32)
    check(getattr(_lib(), entry)(_ptr(xyzs), _ptr(table), _ptr(denc), ctypes.byref(lv), n, _ptr(dxyzs), _stream()), entry)
    return dxyzs


def hash_bwd_input_f32(xyzs, table, denc, lv):
    """d(loss)/d(xyzs) [n,3] of hash_fwd_f32 for d(loss)/d(encoding) = denc [n, L*F]: the derivative of the forward as it evaluates
    (its cell and fraction; on a cell face the cell floorf selects).  Written, not accumulated; bit-reproducible; once differentiable."""
    return _hash_bwd_input("ngp_hash_bwd_input_f32", xyzs, table, torch.float32, denc, torch.float32, lv)


def hash_bwd_input_bf16(xyzs, table_bf16, denc, lv):
    """hash_bwd_input_f32 for hash_fwd_bf16: table_bf16 is the bf16 storage copy the forward gathered from (F = 2)."""
    return _hash_bwd_input("ngp_hash_bwd_input_bf16", xyzs, table_bf16, torch.bfloat16, denc, torch.float32, lv)


def hash_bwd_input_f16(xyzs, table_h, denc_h, lv):
    """hash_bwd_input_f32 for the half2 encoder (hash_fwd_f16): fp16 table [entries, 2], fp16 denc [n, L, 2], f32 arithmetic on the
    forward's f16-rounded cell."""
    return _hash_bwd_input("ngp_hash_bwd_input_f16", xyzs, table_h, torch.float16, denc_h, torch.float16, lv)


# ---------------------------------------------------------------------------------------------------- a-4xx
def _hash_bwd2_check(xyzs, denc, ddx, lv):
    _dev(xyzs, torch.float32, "xyzs"); _dev(denc, torch.float32, "denc"); _dev(ddx, torch.float32, "ddx")
    n = xyzs.shape[0]
    if xyzs.numel() != 3 * n:
        raise ValueError("xyzs must be [n, 3], got %s" % (tuple(xyzs.shape),))
    if denc.numel() != n * lv.n_levels * lv.n_features:
        raise ValueError("denc must hold [n, levels * features] = %d x %d values, got %s"
                         % (n, lv.n_levels * lv.n_features, tuple(denc.shape)))
    if ddx.numel() != 3 * n:
        raise ValueError("ddx must be [n, 3] = [%d, 3], got %s" % (n, tuple(ddx.shape)))
    return n


def _hash_bwd2_gather(entry, xyzs, table, table_dtype, denc, ddx, lv, need_denc, need_x):
    _dev(table, table_dtype, "hash_table")
    n = _hash_bwd2_check(xyzs, denc, ddx, lv)
    if table.numel() != lv.total_entries * lv.n_features:
        raise ValueError("hash_table has %d elements, the level table describes %d" % (table.numel(), lv.total_entries * lv.n_features))
    d_denc = torch.empty(n, lv.n_levels * lv.n_features, device=xyzs.device, dtype=torch.float32) if need_denc else None
    d_x = torch.empty(n, 3, device=xyzs.device, dtype=torch.float32) if need_x else None
    check(getattr(_lib(), entry)(_ptr(xyzs), _ptr(table), _ptr(denc), _ptr(ddx), ctypes.byref(lv), n, _ptr(d_denc), _ptr(d_x), _stream()),
          entry)
    return d_denc, d_x


def hash_bwd2_gather_f32(xyzs, table, denc, ddx, lv, need_denc=True, need_x=True):
    """Double backward of hash_bwd_input_f32 for ddx [n,3] = d(loss)/d(dx): (d_denc [n, L*F] | None, d_x [n,3] | None), the gradients
    with respect to denc and to xyzs.  Written, not accumulated; bit-reproducible; an output that is not needed is not computed."""
    return _hash_bwd2_gather("ngp_hash_bwd2_gather_f32", xyzs, table, torch.float32, denc, ddx, lv, need_denc, need_x)


def hash_bwd2_gather_bf16(xyzs, table_bf16, denc, ddx, lv, need_denc=True, need_x=True):
    """hash_bwd2_gather_f32 for hash_bwd_input_bf16: table_bf16 is the bf16 storage copy the forward gathered from (F = 2)."""
    return _hash_bwd2_gather("ngp_hash_bwd2_gather_bf16", xyzs, table_bf16, torch.bfloat16, denc, ddx, lv, need_denc, need_x)


def hash_bwd2_table_f32(xyzs, denc, ddx, lv, dtable):
    """dtable += the gradient of hash_bwd_input_{f32,bf16}'s dx with respect to the table, for ddx [n,3] = d(loss)/d(dx): the
    scatter-add with scale_l * A_c in place of the trilinear weight.  Float atomics: the summation order is not deterministic."""
    _dev(dtable, torch.float32, "dtable")
    n = _hash_bwd2_check(xyzs, denc, ddx, lv)
    if dtable.numel() != lv.total_entries * lv.n_features:
        raise ValueError("dtable has %d elements, the level table describes %d" % (dtable.numel(), lv.total_entries * lv.n_features))
    check(_lib().ngp_hash_bwd2_table_f32(_ptr(xyzs), _ptr(denc), _ptr(ddx), ctypes.byref(lv), n, _ptr(dtable), _stream()),
          "ngp_hash_bwd2_table_f32")
    _touched(dtable)
    return dtable


# ---------------------------------------------------------------------------------------------------- a-4t
def make_triplane_levels(base_res, max_res, levels, features):
    """ngp_triplane_levels table (host struct) -- TriPlaneEncoder.__init__ arithmetic (triplane.py:103-160)."""
    lv = TriPlaneLevels()
    check(_lib().ngp_triplane_levels_init(ctypes.byref(lv), float(base_res), float(max_res), int(levels), int(features)),
          "ngp_triplane_levels_init")
    return lv


def _norm_args(xyz_min, xyz_max):
    return (0, 0.0, 1.0) if xyz_min is None else (1, float(xyz_min), float(xyz_max))


def triplane_fwd(xyzs, table, lv, xyz_min=None, xyz_max=None):
    """[n,3] positions -> [n, L*F] f32, feature-major (column j*L + level).  Positions in [0,1] (clamped), or in [xyz_min, xyz_max]
    when both are given (the (x - lo) / (hi - lo) of networks.py:144 is then done in the kernel)."""
    _dev(xyzs, torch.float32, "xyzs"); _dev(table, torch.float32, "plane_embedding")
    if table.numel() != 3 * lv.max_res**2 * lv.n_features:
        raise ValueError("plane_embedding has %d floats, the level table needs %d" % (table.numel(), 3 * lv.max_res**2 * lv.n_features))
    n = xyzs.shape[0]
    out = torch.empty(n, lv.n_levels * lv.n_features, device=xyzs.device, dtype=torch.float32)
    check(_lib().ngp_triplane_fwd_f32(_ptr(xyzs), _ptr(table), ctypes.byref(lv), n, *_norm_args(xyz_min, xyz_max), _ptr(out), _stream()),
          "ngp_triplane_fwd_f32")
    return out


def triplane_bwd(xyzs, dout, table, lv, dtable, xyz_min=None, xyz_max=None):
    """dtable += d(encoding)/d(table)^T dout: the true gradient of triplane_fwd (it depends on `table`)."""
    _dev(xyzs, torch.float32, "xyzs"); _dev(dout, torch.float32, "dout"); _dev(table, torch.float32, "plane_embedding")
    _dev(dtable, torch.float32, "dtable")
    if dtable.numel() != table.numel() or dout.shape != (xyzs.shape[0], lv.n_levels * lv.n_features):
        raise ValueError("triplane_bwd: dtable must match the table, dout must be [n, L*F]")
    check(_lib().ngp_triplane_bwd_f32(_ptr(xyzs), _ptr(dout), _ptr(table), ctypes.byref(lv), xyzs.shape[0], *_norm_args(xyz_min, xyz_max),
                                      _ptr(dtable), _stream()), "ngp_triplane_bwd_f32")
    _touched(dtable)
    return dtable


# ---------------------------------------------------------------------------------------------------- a-4v
def _voxel_fields(sh, density, grid_size, sh_degree):
    _dev(sh, torch.float32, "sh_fields"); _dev(density, torch.float32, "density_fields")
    G, D = int(grid_size), (int(sh_degree) + 1)**2
    if sh.numel() != G**3 * 3 * D or density.numel() != G**3:
        raise ValueError("voxel fields must be [G,G,G,3*D] and [G,G,G,1] for G=%d, degree %d" % (G, sh_degree))


def voxel_fwd(xyzs, dirs, sh, density, grid_size, sh_degree, grid_min, grid_radius, trilinear=False):
    """positions [n,3], directions [n,3] -> (sigmas [n], rgbs [n,3]): nearest voxel of (p - grid_min) / grid_radius (trilinear: the
    eight surrounding grid points interpolated, zero outside the grid), relu density, sigmoid of eval_sh per channel (VoxelGrid,
    modules/networks.py)."""
    _dev(xyzs, torch.float32, "xyzs"); _dev(dirs, torch.float32, "dirs")
    _voxel_fields(sh, density, grid_size, sh_degree)
    n = xyzs.shape[0]
    if xyzs.shape != (n, 3) or dirs.shape != (n, 3):
        raise ValueError("voxel_fwd: xyzs and dirs must both be [n, 3], got %s and %s" % (tuple(xyzs.shape), tuple(dirs.shape)))
    sigmas = torch.empty(n, device=xyzs.device, dtype=torch.float32)
    rgbs = torch.empty(n, 3, device=xyzs.device, dtype=torch.float32)
    name = "ngp_voxel_trilinear_fwd" if trilinear else "ngp_voxel_fwd"
    check(getattr(_lib(), name)(_ptr(xyzs), _ptr(dirs), _ptr(sh), _ptr(density), n, int(grid_size), int(sh_degree), float(grid_min),
                                float(grid_radius), _ptr(sigmas), _ptr(rgbs), _stream()), name)
    return sigmas, rgbs


def voxel_density(xyzs, density, grid_size, grid_min, grid_radius, out=None, trilinear=False):
    _dev(xyzs, torch.float32, "xyzs"); _dev(density, torch.float32, "density_fields")
    if density.numel() != int(grid_size)**3:
        raise ValueError("density_fields must hold G^3 values")
    n = xyzs.shape[0]
    if xyzs.shape != (n, 3) or (out is not None and (out.shape != (n,) or not out.is_contiguous() or out.dtype != torch.float32)):
        raise ValueError("voxel_density: xyzs must be [n, 3] and out a contiguous f32 [n]")
    sigmas = torch.empty(n, device=xyzs.device, dtype=torch.float32) if out is None else out
    name = "ngp_voxel_trilinear_density" if trilinear else "ngp_voxel_density"
    check(getattr(_lib(), name)(_ptr(xyzs), _ptr(density), n, int(grid_size), float(grid_min), float(grid_radius), _ptr(sigmas),
                                _stream()), name)
    return sigmas


def voxel_bwd(xyzs, dirs, sigmas, rgbs, dsigmas, drgbs, grid_size, sh_degree, grid_min, grid_radius, dsh, ddensity, trilinear=False):
    """dsh += d loss / d sh_fields, ddensity += d loss / d density_fields (both zero-filled by the caller); trilinear: of the forward
    with trilinear=True."""
    for t, name in ((xyzs, "xyzs"), (dirs, "dirs"), (sigmas, "sigmas"), (rgbs, "rgbs"), (dsigmas, "dsigmas"), (drgbs, "drgbs")):
        _dev(t, torch.float32, name)
    _voxel_fields(dsh, ddensity, grid_size, sh_degree)
    n = xyzs.shape[0]
    if dirs.shape != (n, 3) or sigmas.shape != (n,) or rgbs.shape != (n, 3) or dsigmas.shape != (n,) or drgbs.shape != (n, 3):
        raise ValueError("voxel_bwd: per-sample tensors must be [n], [n,3]")
    name = "ngp_voxel_trilinear_bwd" if trilinear else "ngp_voxel_bwd"
    check(getattr(_lib(), name)(_ptr(xyzs), _ptr(dirs), _ptr(sigmas), _ptr(rgbs), _ptr(dsigmas), _ptr(drgbs), n, int(grid_size),
                                int(sh_degree), float(grid_min), float(grid_radius), _ptr(dsh), _ptr(ddensity), _stream()), name)
    _touched(dsh, ddensity)
    return dsh, ddensity


def voxel_occ_pack(density_grid, density_threshold, density_bitfield, scratch=None):
    """bit = density >= min(f64 mean of the positive cells, density_threshold) and density > 0 (VoxelGrid.update_density_grid).
    The kernel reads density_grid as float4: it must start on a 16-byte boundary (a fresh torch allocation does)."""
    _dev(density_grid, torch.float32, "density_grid"); _dev(density_bitfield, torch.uint8, "density_bitfield")
    n_bytes = density_bitfield.numel()
    if density_grid.numel() != 8 * n_bytes:
        raise ValueError("density_grid must hold 8 cells per bitfield byte")
    if density_grid.data_ptr() % 16:
        raise ValueError("density_grid must start on a 16-byte boundary (the packing kernel reads float4)")
    if scratch is not None and (scratch.dtype != torch.float64 or not scratch.is_cuda
                                or scratch.numel() < _lib().ngp_voxel_occ_scratch_doubles()):
        raise ValueError("scratch must be a device f64 buffer of ngp_voxel_occ_scratch_doubles() values")
    if scratch is None:
        scratch = torch.empty(_lib().ngp_voxel_occ_scratch_doubles(), device=density_grid.device, dtype=torch.float64)
    check(_lib().ngp_voxel_occ_pack(_ptr(density_grid), n_bytes, float(density_threshold), _ptr(scratch), _ptr(density_bitfield),
                                    _stream()), "ngp_voxel_occ_pack")
    _touched(density_bitfield)
    return density_bitfield


# ---------------------------------------------------------------------------------------------------- a-4d
def deploy_shade(xyzs, dirs, table, lv, sigma_w, rgb_w, return_enc=False):
    """The deployment model's shading in one launch (ngp_deploy_shade): world positions [n,3] in [-0.5, 0.5] and directions [n,3]
    -> (sigmas [n], rgbs [n,3]) f32, plus the [n,16] embedding with return_enc=True (tests).  table: fp32 [entries * 4] of the level
    table `lv` = make_levels(2**21, 4, 32, 128, 4); sigma_w [512], rgb_w [768] in save_deployment_model's layout."""
    for t, name in ((xyzs, "xyzs"), (dirs, "dirs"), (table, "hash_table"), (sigma_w, "sigma_weights"), (rgb_w, "rgb_weights")):
        _dev(t, torch.float32, name)
    n = xyzs.shape[0]
    if xyzs.shape != (n, 3) or dirs.shape != (n, 3):
        raise ValueError("deploy_shade: xyzs and dirs must both be [n, 3], got %s and %s" % (tuple(xyzs.shape), tuple(dirs.shape)))
    if lv.n_levels != 4 or lv.n_features != 4 or lv.begin_fast_hash_level != 4:
        raise ValueError("deploy_shade needs the deployment level table: 4 dense levels of 4 features")
    if table.numel() != lv.total_entries * 4 or sigma_w.numel() != 512 or rgb_w.numel() != 768:
        raise ValueError("deploy_shade: table must hold %d floats, sigma_weights 512, rgb_weights 768 (got %d, %d, %d)"
                         % (lv.total_entries * 4, table.numel(), sigma_w.numel(), rgb_w.numel()))
    sigmas = torch.empty(n, device=xyzs.device, dtype=torch.float32)
    rgbs = torch.empty(n, 3, device=xyzs.device, dtype=torch.float32)
    enc = torch.empty(n, 16, device=xyzs.device, dtype=torch.float32) if return_enc else None
    check(_lib().ngp_deploy_shade(_ptr(xyzs), _ptr(dirs), _ptr(table), ctypes.byref(lv), _ptr(sigma_w), _ptr(rgb_w), n, _ptr(sigmas),
                                  _ptr(rgbs), _ptr(enc), _stream()), "ngp_deploy_shade")
    return (sigmas, rgbs, enc) if return_enc else (sigmas, rgbs)


def deploy_render(rays_o, rays_d, density_bitfield, coarse, table, lv, sigma_w, rgb_w, T_threshold=1e-2, max_samples=1024, out=None):
    """Rays of a deployment model to pixels in one launch (ngp_deploy_render): slab test, occupancy march, shading and front-to-back
    compositing per ray, the march ending where the composite does.  rays_o, rays_d [n,3] f32; density_bitfield: the 262 144 uint8 of the
    one 128^3 cascade; coarse: coarse_bitfield(density_bitfield, 1, 128) (int32 [128]) or None; table, lv, sigma_w, rgb_w as for
    deploy_shade.  -> (rgb [n,3], opacity [n], depth [n], n_samples [n] int32, t_last [n]); `out` = that tuple preallocated.
    Shapes and dtypes are checked first (ValueError), then that everything lives on the GPU."""
    f32, n = torch.float32, rays_o.shape[0]
    want = [(rays_o, "rays_o", f32, (n, 3)), (rays_d, "rays_d", f32, (n, 3)), (table, "hash_table", f32, (lv.total_entries * 4,)),
            (sigma_w, "sigma_weights", f32, (512,)), (rgb_w, "rgb_weights", f32, (768,)),
            (density_bitfield, "density_bitfield", torch.uint8, (128**3 // 8,))]
    if coarse is not None:
        want.append((coarse, "coarse", torch.int32, (128**3 // 512 // 32,)))          # coarse_bitfield(density_bitfield, 1, 128)
    if out is not None:
        rgb, opacity, depth, n_samples, t_last = out
        want += [(rgb, "out rgb", f32, (n, 3)), (opacity, "out opacity", f32, (n,)), (depth, "out depth", f32, (n,)),
                 (n_samples, "out n_samples", torch.int32, (n,)), (t_last, "out t_last", f32, (n,))]
    if lv.n_levels != 4 or lv.n_features != 4 or lv.begin_fast_hash_level != 4:
        raise ValueError("deploy_render needs the deployment level table: 4 dense levels of 4 features")
    for t, name, dt, shape in want:
        if t.dtype != dt or tuple(t.shape) != shape:
            raise ValueError("deploy_render: %s must be %s %s, got %s %s" % (name, dt, shape, t.dtype, tuple(t.shape)))
    if table.data_ptr() % 16:
        raise ValueError("deploy_render: the hash table must be 16-byte aligned")
    if int(max_samples) < 1:
        raise ValueError("deploy_render: max_samples must be at least 1, got %r" % (max_samples,))
    for t, name, dt, _ in want:
        _dev(t, dt, name)
    if out is None:
        dev = rays_o.device
        out = (torch.empty(n, 3, device=dev), torch.empty(n, device=dev), torch.empty(n, device=dev),
               torch.empty(n, device=dev, dtype=torch.int32), torch.empty(n, device=dev))
    rgb, opacity, depth, n_samples, t_last = out
    check(_lib().ngp_deploy_render(_ptr(rays_o), _ptr(rays_d), _ptr(density_bitfield), _ptr(coarse), _ptr(table), ctypes.byref(lv),
                                   _ptr(sigma_w), _ptr(rgb_w), n, int(max_samples), float(T_threshold), _ptr(rgb), _ptr(opacity), _ptr(depth),
                                   _ptr(n_samples), _ptr(t_last), _stream()), "ngp_deploy_render")
    _touched(*out)
    return out


# ---------------------------------------------------------------------------------------------------- a-6
def sh16_fwd(dirs):
    _dev(dirs, torch.float32, "dirs")
    out = torch.empty(dirs.shape[0], 16, device=dirs.device, dtype=torch.float32)
    check(_lib().ngp_sh16_fwd(_ptr(dirs), dirs.shape[0], _ptr(out), _stream()), "ngp_sh16_fwd")
    return out


def sh16_bwd(dirs, dout):
    _dev(dirs, torch.float32, "dirs"); _dev(dout, torch.float32, "dout")
    ddirs = torch.empty_like(dirs)
    check(_lib().ngp_sh16_bwd(_ptr(dirs), _ptr(dout), dirs.shape[0], _ptr(ddirs), _stream()), "ngp_sh16_bwd")
    return ddirs


# ---------------------------------------------------------------------------------------------------- a-7
def _rgb_kind(rgbs):
    if rgbs.dtype == torch.float16:
        return 1
    if rgbs.dtype == torch.float32:
        return 0
    raise TypeError("rgbs must be float16 or float32, got %s" % rgbs.dtype)


def composite_train_fwd(sigmas, rgbs, deltas, ts, rays_a, T_threshold):
    _dev(sigmas, torch.float32, "sigmas"); _dev(rgbs, None, "rgbs"); _dev(deltas, torch.float32, "deltas")
    _dev(ts, torch.float32, "ts"); _dev(rays_a, torch.int32, "rays_a")
    n = rays_a.shape[0]
    dev = rays_a.device
    total_samples = torch.empty(n, device=dev, dtype=torch.int32)
    opacity = torch.empty(n, device=dev, dtype=torch.float32)
    depth = torch.empty(n, device=dev, dtype=torch.float32)
    rgb = torch.empty(n, 3, device=dev, dtype=torch.float32)
    ws = torch.empty_like(sigmas)
    check(_lib().ngp_composite_train_fwd(_ptr(sigmas), _ptr(rgbs), _rgb_kind(rgbs), _ptr(deltas), _ptr(ts), _ptr(rays_a),
                                         float(T_threshold), n, _ptr(total_samples), _ptr(opacity), _ptr(depth), _ptr(rgb),
                                         _ptr(ws), _stream()), "ngp_composite_train_fwd")
    return total_samples, opacity, depth, rgb, ws


def composite_train_bwd(dL_dopacity, dL_ddepth, dL_drgb, dL_dws, sigmas, rgbs, deltas, ts, rays_a, opacity, depth, rgb, ws,
                        T_threshold):
    n = rays_a.shape[0]
    for name, t in (("dL_dopacity", dL_dopacity), ("dL_ddepth", dL_ddepth), ("dL_drgb", dL_drgb), ("dL_dws", dL_dws)):
        if t is not None:
            _dev(t, torch.float32, name)
    d_sigmas = torch.empty_like(sigmas)
    d_rgbs = torch.empty_like(rgbs)
    check(_lib().ngp_composite_train_bwd(_ptr(dL_dopacity), _ptr(dL_ddepth), _ptr(dL_drgb), _ptr(dL_dws), _ptr(sigmas),
                                         _ptr(rgbs), _rgb_kind(rgbs), _ptr(deltas), _ptr(ts), _ptr(rays_a), _ptr(opacity),
                                         _ptr(depth), _ptr(rgb), _ptr(ws), float(T_threshold), n, _ptr(d_sigmas), _ptr(d_rgbs),
                                         _stream()), "ngp_composite_train_bwd")
    return d_sigmas, d_rgbs


# ---------------------------------------------------------------------------------------------------- a-8
def composite_test(sigmas, rgbs, deltas, ts, pack_info, alive_indices, T_threshold, opacity, depth, rgb):
    _dev(sigmas, torch.float32, "sigmas"); _dev(rgbs, None, "rgbs"); _dev(deltas, torch.float32, "deltas")
    _dev(ts, torch.float32, "ts"); _dev(pack_info, torch.int64, "pack_info"); _dev(alive_indices, torch.int64, "alive_indices")
    _dev(opacity, torch.float32, "opacity"); _dev(depth, torch.float32, "depth"); _dev(rgb, torch.float32, "rgb")
    check(_lib().ngp_composite_test(_ptr(sigmas), _ptr(rgbs), _rgb_kind(rgbs), _ptr(deltas), _ptr(ts), _ptr(pack_info),
                                    _ptr(alive_indices), float(T_threshold), alive_indices.shape[0], _ptr(opacity), _ptr(depth),
                                    _ptr(rgb), _stream()), "ngp_composite_test")
    _touched(opacity, depth, rgb, alive_indices)


# ---------------------------------------------------------------------------------------------------- a-9
MLP_N_WEIGHTS = 2048 + 1024 + 2048 + 4096 + 192
MLP_SPLITS = (2048, 1024, 2048, 4096, 192)
MLP_SHAPES = ((64, 32), (16, 64), (64, 32), (64, 64), (3, 64))


def mlp_pack(weights):
    """weights: the five fp32 nn.Linear weight tensors (W1 [64,32], W2 [16,64], W3 [64,32], W4 [64,64], W5 [3,64])
    -> fp16 MFMA-fragment image consumed by mlp_fwd / mlp_bwd."""
    ws = []
    for w, shape in zip(weights, MLP_SHAPES):
        if tuple(w.shape) != shape:
            raise ValueError("fused MLP needs the default architecture; got weight shape %s, want %s" % (tuple(w.shape), shape))
        ws.append(_dev(w.detach().contiguous(), torch.float32, "mlp weight"))
    wpack = torch.empty(_lib().ngp_mlp_wpack_halfs(), device=ws[0].device, dtype=torch.float16)
    check(_lib().ngp_mlp_pack(*[_ptr(w) for w in ws], 0, _ptr(wpack), _stream()), "ngp_mlp_pack")
    return wpack


def mlp_fwd(enc, dirs, wpack):
    """enc [n,32] f32, dirs [n,3] f32 (raw directions) -> (sigmas [n] f32, rgbs [n,3] f16)."""
    _dev(enc, torch.float32, "enc"); _dev(dirs, torch.float32, "dirs"); _dev(wpack, torch.float16, "wpack")
    n = enc.shape[0]
    sigmas = torch.empty(n, device=enc.device, dtype=torch.float32)
    rgbs = torch.empty(n, 3, device=enc.device, dtype=torch.float16)
    check(_lib().ngp_mlp_fwd(_ptr(enc), _ptr(dirs), _ptr(wpack), n, _ptr(sigmas), _ptr(rgbs), _stream()), "ngp_mlp_fwd")
    return sigmas, rgbs


def mlp_density(enc, wpack):
    """density head only: enc [n,32] f32 -> sigmas [n] f32."""
    _dev(enc, torch.float32, "enc"); _dev(wpack, torch.float16, "wpack")
    n = enc.shape[0]
    sigmas = torch.empty(n, device=enc.device, dtype=torch.float32)
    check(_lib().ngp_mlp_fwd(_ptr(enc), _ptr(None), _ptr(wpack), n, _ptr(sigmas), _ptr(None), _stream()), "ngp_mlp_fwd")
    return sigmas


def mlp_bwd(enc, dirs, wpack, dsigmas, drgbs):
    """-> (d_enc [n,32] f32, dW [9408] f32 flat = W1|W2|W3|W4|W5)."""
    _dev(enc, torch.float32, "enc"); _dev(dirs, torch.float32, "dirs"); _dev(wpack, torch.float16, "wpack")
    _dev(dsigmas, torch.float32, "dsigmas"); _dev(drgbs, torch.float16, "drgbs")
    n = enc.shape[0]
    d_enc = torch.empty_like(enc)
    dW = torch.zeros(MLP_N_WEIGHTS, device=enc.device, dtype=torch.float32)
    check(_lib().ngp_mlp_bwd(_ptr(enc), _ptr(dirs), _ptr(wpack), _ptr(dsigmas), _ptr(drgbs), n, _ptr(d_enc), _ptr(dW), _stream()),
          "ngp_mlp_bwd")
    return d_enc, dW


# ---------------------------------------------------------------------------------------------------- a-10
def morton3d(coords):
    _dev(coords, torch.int32, "coords")
    out = torch.empty(coords.shape[0], device=coords.device, dtype=torch.int32)
    check(_lib().ngp_morton3d(_ptr(coords), coords.shape[0], _ptr(out), _stream()), "ngp_morton3d")
    return out


def morton3d_invert(indices):
    _dev(indices, torch.int32, "indices")
    out = torch.empty(indices.shape[0], 3, device=indices.device, dtype=torch.int32)
    check(_lib().ngp_morton3d_invert(_ptr(indices), indices.shape[0], _ptr(out), _stream()), "ngp_morton3d_invert")
    return out


def packbits(density_grid, threshold, density_bitfield):
    _dev(density_grid, torch.float32, "density_grid"); _dev(density_bitfield, torch.uint8, "density_bitfield")
    n_bytes = density_bitfield.shape[0]
    if density_grid.numel() != 8 * n_bytes:
        raise ValueError("density_grid must hold 8 floats per bitfield byte")
    check(_lib().ngp_packbits(_ptr(density_grid), float(threshold), n_bytes, _ptr(density_bitfield), _stream()), "ngp_packbits")
    _touched(density_bitfield)
    return density_bitfield


# ---------------------------------------------------------------------------------------------------- f-1
def distortion_fwd(ws, deltas, ts, rays_a):
    _dev(ws, torch.float32, "ws"); _dev(deltas, torch.float32, "deltas"); _dev(ts, torch.float32, "ts")
    _dev(rays_a, torch.int32, "rays_a")
    n = rays_a.shape[0]
    loss = torch.zeros(n, device=ws.device, dtype=torch.float32)
    ws_inc = torch.empty_like(ws)
    wts_inc = torch.empty_like(ws)
    check(_lib().ngp_distortion_fwd(_ptr(ws), _ptr(deltas), _ptr(ts), _ptr(rays_a), n, _ptr(loss), _ptr(ws_inc), _ptr(wts_inc),
                                    _stream()), "ngp_distortion_fwd")
    return loss, ws_inc, wts_inc


def distortion_bwd(dL_dloss, ws, deltas, ts, ws_inc, wts_inc, rays_a):
    _dev(dL_dloss, torch.float32, "dL_dloss")
    dL_dws = torch.zeros_like(ws)
    check(_lib().ngp_distortion_bwd(_ptr(dL_dloss), _ptr(ws), _ptr(deltas), _ptr(ts), _ptr(ws_inc), _ptr(wts_inc), _ptr(rays_a),
                                    rays_a.shape[0], _ptr(dL_dws), _stream()), "ngp_distortion_bwd")
    return dL_dws


# ---------------------------------------------------------------------------------------------------- isosurface extraction
def _mesh_grid(values, sign):
    """Shape and sign checks first (they need no device), then the device check."""
    if values.dim() != 3 or min(values.shape) < 2:
        raise ValueError("values must be [Nx, Ny, Nz] with every N >= 2, got %s" % (tuple(values.shape),))
    if values.numel() >= 2**31:
        raise ValueError("values holds %d points; the extraction indexes them with int32 (< 2^31)" % values.numel())
    if sign not in (1, -1):
        raise ValueError("sign must be +1 (inside = above iso, a density) or -1 (inside = below iso, a signed distance), got %r" % (sign,))
    _dev(values, torch.float32, "values")
    return tuple(int(s) for s in values.shape)


def mesh_count(values, iso, sign=1, workspace=None):
    """First phase of marching tetrahedra on values [Nx, Ny, Nz] (csrc/mesh.hip): -> (workspace uint8 [ngp_mesh_workspace_bytes],
    counts int32 [2] = {vertices, faces}, ON THE DEVICE).  The workspace is what mesh_emit needs; pass one back in to reuse it."""
    nx, ny, nz = _mesh_grid(values, sign)
    need = _lib().ngp_mesh_workspace_bytes(nx, ny, nz)
    if workspace is None:
        workspace = torch.empty(need, device=values.device, dtype=torch.uint8)
    elif not workspace.is_cuda or workspace.dtype != torch.uint8 or workspace.numel() < need or not workspace.is_contiguous():
        raise ValueError("workspace must be a contiguous device uint8 buffer of at least %d bytes" % need)
    counts = torch.empty(2, device=values.device, dtype=torch.int32)
    check(_lib().ngp_mesh_count(_ptr(values), nx, ny, nz, float(iso), int(sign), _ptr(workspace), _ptr(counts), _stream()),
          "ngp_mesh_count")
    return workspace, counts


def mesh_emit(values, iso, sign, lo, h, workspace, n_vertices, n_faces, normals=True):
    """Second phase, after mesh_count on the same values, iso and sign: -> (vertices f32 [V,3], normals f32 [V,3] or None, faces int32
    [T,3]).  n_vertices, n_faces: the host copies of mesh_count's counts.  lo, h: three floats each, h > 0."""
    lo, h = [float(x) for x in lo], [float(x) for x in h]
    if len(lo) != 3 or len(h) != 3 or not all(x > 0 for x in h):
        raise ValueError("lo and h must hold three floats each and every h must be positive, got lo=%r h=%r" % (lo, h))
    nx, ny, nz = _mesh_grid(values, sign)
    if n_vertices < 0 or n_faces < 0:
        raise ValueError("the mesh has more than 2^31 - 1 vertices or faces: extract it in parts")
    _dev(workspace, torch.uint8, "workspace")
    if workspace.numel() < _lib().ngp_mesh_workspace_bytes(nx, ny, nz):
        raise ValueError("workspace is smaller than ngp_mesh_workspace_bytes of this grid")
    vertices = torch.empty(n_vertices, 3, device=values.device, dtype=torch.float32)
    faces = torch.empty(n_faces, 3, device=values.device, dtype=torch.int32)
    nrm = torch.empty(n_vertices, 3, device=values.device, dtype=torch.float32) if normals else None
    if n_vertices == 0 or n_faces == 0:                  # nothing to write: no launch
        return vertices, nrm, faces
    check(_lib().ngp_mesh_emit(_ptr(values), nx, ny, nz, float(iso), int(sign), (ctypes.c_float * 3)(*lo), (ctypes.c_float * 3)(*h),
                               _ptr(workspace), _ptr(vertices), _ptr(nrm), _ptr(faces), _stream()), "ngp_mesh_emit")
    return vertices, nrm, faces


# ---------------------------------------------------------------------------------------------------- distance to a triangle mesh
MESH_SDF_MAX_LEAF = _lib_mod._ABI.defines["NGP_MESH_SDF_MAX_LEAF"]


def _mesh_sdf_mesh(vertices, faces, order, leaf_size, boxes=None):
    """Shapes first (no device needed), then the devices -> (n_faces in the tree, bytes of its boxes); boxes, where given, must be that
    tree's."""
    if vertices.dim() != 2 or vertices.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3 or order.dim() != 1:
        raise ValueError("vertices must be [V,3], faces [T,3] and order [n_faces], got %s, %s, %s"
                         % (tuple(vertices.shape), tuple(faces.shape), tuple(order.shape)))
    if not 1 <= int(leaf_size) <= MESH_SDF_MAX_LEAF:
        raise ValueError("leaf_size must be in 1..%d, got %r" % (MESH_SDF_MAX_LEAF, leaf_size))
    if not 1 <= order.shape[0] <= faces.shape[0]:
        raise ValueError("order must name between one and all of the %d faces, got %d" % (faces.shape[0], order.shape[0]))
    _dev(vertices, torch.float32, "vertices"); _dev(faces, torch.int32, "faces"); _dev(order, torch.int32, "order")
    need = _lib().ngp_mesh_bvh_bytes(order.shape[0], int(leaf_size))
    if need < 0:
        raise ValueError("%d faces in leaves of %d make a tree deeper than the walk's 24 levels: use a larger leaf_size"
                         % (order.shape[0], leaf_size))
    if boxes is not None:
        _dev(boxes, torch.float32, "boxes")
        if boxes.numel() * 4 != need:
            raise ValueError("boxes holds %d bytes, the tree of %d faces in leaves of %d needs %d"
                             % (boxes.numel() * 4, order.shape[0], leaf_size, need))
    return int(order.shape[0]), need


def mesh_bvh_build(vertices, faces, order, leaf_size=4):
    """The box hierarchy of csrc/mesh_sdf.hip over the faces order [n_faces] names (rows of faces [T,3] int32, indices into vertices
    [V,3] f32: TRUSTED, the caller has checked their range), in that order -> boxes f32 [2 P - 1, 6]."""
    n_faces, need = _mesh_sdf_mesh(vertices, faces, order, leaf_size)
    boxes = torch.empty(need // 24, 6, device=vertices.device, dtype=torch.float32)
    check(_lib().ngp_mesh_bvh_build(_ptr(vertices), _ptr(faces), _ptr(order), n_faces, int(leaf_size), _ptr(boxes), _stream()),
          "ngp_mesh_bvh_build")
    return boxes


def mesh_sdf_query(points, vertices, faces, order, boxes, leaf_size=4, edge_normals=None, vertex_normals=None, details=True):
    """Nearest face of every point [n,3] f32 -> (sdf [n], closest [n,3], face [n] int32, feature [n] int32); details=False: only sdf, the
    others None (the same bits).  Signed iff edge_normals f32 [T,3,3] and vertex_normals f32 [V,3] are given (both or neither)."""
    n_faces, _ = _mesh_sdf_mesh(vertices, faces, order, leaf_size, boxes)
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError("points must be [n,3], got %s" % (tuple(points.shape),))
    if (edge_normals is None) != (vertex_normals is None):
        raise ValueError("edge_normals and vertex_normals go together: both for the signed distance, neither for the unsigned")
    _dev(points, torch.float32, "points")
    if edge_normals is not None:
        _dev(edge_normals, torch.float32, "edge_normals"); _dev(vertex_normals, torch.float32, "vertex_normals")
        if tuple(edge_normals.shape) != (faces.shape[0], 3, 3) or tuple(vertex_normals.shape) != tuple(vertices.shape):
            raise ValueError("edge_normals must be [T,3,3] and vertex_normals [V,3]")
    n = points.shape[0]
    sdf = torch.empty(n, device=points.device, dtype=torch.float32)
    closest = torch.empty(n, 3, device=points.device, dtype=torch.float32) if details else None
    face = torch.empty(n, device=points.device, dtype=torch.int32) if details else None
    feature = torch.empty(n, device=points.device, dtype=torch.int32) if details else None
    check(_lib().ngp_mesh_sdf_query(_ptr(points), n, _ptr(vertices), _ptr(faces), _ptr(order), _ptr(boxes), n_faces, int(leaf_size),
                                    _ptr(edge_normals), _ptr(vertex_normals), _ptr(sdf), _ptr(closest), _ptr(face), _ptr(feature),
                                    _stream()), "ngp_mesh_sdf_query")
    return sdf, closest, face, feature


RAYCAST_ANY_HIT, RAYCAST_CULL_BACK, RAYCAST_CULL_FRONT = (_lib_mod._ABI.defines[k] for k in
                                                          ("NGP_RAYCAST_ANY_HIT", "NGP_RAYCAST_CULL_BACK", "NGP_RAYCAST_CULL_FRONT"))


def mesh_raycast(rays_o, rays_d, vertices, faces, order, boxes, leaf_size=4, t_min=0.0, t_max=float("inf"), any_hit=False, cull=None,
                 details=True):
    """First face along every ray o + t d (csrc/mesh_raycast.hip), rays_o / rays_d [n,3] f32, in the tree of mesh_bvh_build -> (t [n]: +inf
    on a miss, face [n] int32: -1, bary [n,2]: 0, side [n] int32: +1 front, -1 back, 0 miss); details=False: only t, the others None (the
    same bits).  t in [t_min, t_max], in units of |d|.  any_hit: stop at the first accepted face (occlusion).  cull: None, "back" or
    "front"."""
    n_faces, _ = _mesh_sdf_mesh(vertices, faces, order, leaf_size, boxes)
    if rays_o.dim() != 2 or rays_o.shape[1] != 3 or tuple(rays_d.shape) != tuple(rays_o.shape):
        raise ValueError("rays_o and rays_d must both be [n,3], got %s and %s" % (tuple(rays_o.shape), tuple(rays_d.shape)))
    if cull not in (None, "back", "front"):
        raise ValueError("cull must be None, 'back' or 'front', got %r" % (cull,))
    _dev(rays_o, torch.float32, "rays_o"); _dev(rays_d, torch.float32, "rays_d")
    flags = (RAYCAST_ANY_HIT if any_hit else 0) | {None: 0, "back": RAYCAST_CULL_BACK, "front": RAYCAST_CULL_FRONT}[cull]
    n, dev = rays_o.shape[0], rays_o.device
    t = torch.empty(n, device=dev, dtype=torch.float32)
    face = torch.empty(n, device=dev, dtype=torch.int32) if details else None
    bary = torch.empty(n, 2, device=dev, dtype=torch.float32) if details else None
    side = torch.empty(n, device=dev, dtype=torch.int32) if details else None
    check(_lib().ngp_mesh_raycast(_ptr(rays_o), _ptr(rays_d), n, _ptr(vertices), _ptr(faces), _ptr(order), _ptr(boxes), n_faces,
                                  int(leaf_size), float(t_min), float(t_max), flags, _ptr(t), _ptr(face), _ptr(bary), _ptr(side), _stream()),
          "ngp_mesh_raycast")
    return t, face, bary, side


MESH_WINDING_ROW = 20        # floats per node of `moments` (include/ngp_hip.h publishes the columns)


def _mesh_winding_bytes(n_faces, leaf_size):
    need = _lib().ngp_mesh_winding_bytes(n_faces, int(leaf_size))
    if need < 0:
        raise ValueError("%d faces in leaves of %d make a tree the winding number refuses" % (n_faces, leaf_size))
    return need


def mesh_winding_build(vertices, faces, order, boxes, leaf_size=4):
    """The per-node moments of csrc/mesh_winding.hip (centroid, radius, area vector, area, second-order tensor) over the tree of
    mesh_bvh_build -> moments f32 [2 P - 1, 20]."""
    n_faces, _ = _mesh_sdf_mesh(vertices, faces, order, leaf_size, boxes)
    moments = torch.empty(_mesh_winding_bytes(n_faces, leaf_size) // (4 * MESH_WINDING_ROW), MESH_WINDING_ROW, device=vertices.device,
                          dtype=torch.float32)
    check(_lib().ngp_mesh_winding_build(_ptr(vertices), _ptr(faces), _ptr(order), _ptr(boxes), n_faces, int(leaf_size), _ptr(moments),
                                        _stream()), "ngp_mesh_winding_build")
    return moments


def mesh_winding_query(points, vertices, faces, order, moments, leaf_size=4, beta=2.0, order_terms=2):
    """Generalized winding number of every point [n,3] f32 against the mesh (csrc/mesh_winding.hip) -> w [n] f32: 1 inside a closed,
    outward-oriented mesh, 0 outside, in between near holes.  A node of the tree farther than beta x its radius is replaced by its
    expansion of order_terms (1 or 2); beta >= 1, beta = inf: the exact sum over all faces."""
    n_faces, _ = _mesh_sdf_mesh(vertices, faces, order, leaf_size)
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError("points must be [n,3], got %s" % (tuple(points.shape),))
    if not float(beta) >= 1.0:
        raise ValueError("beta must be at least 1 (a node is accepted only from outside its radius), got %r" % (beta,))
    if order_terms not in (1, 2):
        raise ValueError("order_terms must be 1 or 2, got %r" % (order_terms,))
    _dev(points, torch.float32, "points"); _dev(moments, torch.float32, "moments")
    need = _mesh_winding_bytes(n_faces, leaf_size)
    if moments.numel() * 4 != need:
        raise ValueError("moments holds %d bytes, the tree of %d faces in leaves of %d needs %d" % (moments.numel() * 4, n_faces, leaf_size, need))
    if moments.data_ptr() % 16:
        raise ValueError("moments must start at a multiple of 16 bytes: the query reads its rows as 16-byte vectors")
    n = points.shape[0]
    winding = torch.empty(n, device=points.device, dtype=torch.float32)
    check(_lib().ngp_mesh_winding_query(_ptr(points), n, _ptr(vertices), _ptr(faces), _ptr(order), _ptr(moments), n_faces, int(leaf_size),
                                        float(beta), int(order_terms), _ptr(winding), _stream()), "ngp_mesh_winding_query")
    return winding


# ---------------------------------------------------------------------------------------------------- connected components of a mesh
MESH_COMPONENTS_BATCH = 4      # union-find rounds per host read of the `changed` flags
MESH_TABLE_COLUMNS = ("vertices", "faces", "edges", "boundary_edges", "nonmanifold_edges", "euler")


def _mesh_faces(faces, n_vertices):
    if faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError("faces must be [T,3], got %s" % (tuple(faces.shape),))
    n_vertices = int(n_vertices)
    if not 0 <= n_vertices < 2**31:
        raise ValueError("n_vertices must be in 0..2^31 - 1, got %r" % (n_vertices,))
    _dev(faces, torch.int32, "faces")
    return int(faces.shape[0]), n_vertices


def _mesh_arrays(vertices, faces=None):
    """The checks every mesh entry makes of its vertices f32 [V,3] and, where it takes them, its faces -> (T, V); T = 0 without faces."""
    if vertices.dim() != 2 or vertices.shape[1] != 3:
        raise ValueError("vertices must be [V,3], got %s" % (tuple(vertices.shape),))
    _dev(vertices, torch.float32, "vertices")
    return _mesh_faces(faces, vertices.shape[0]) if faces is not None else (0, int(vertices.shape[0]))


def _mesh_mask(mask, name):
    """A per-component or per-vertex mask (uint8 / bool, on the device) as the kernels read it."""
    if not mask.is_cuda:
        raise RuntimeError("%s must live on the GPU: libngp_hip has no CPU path (got device %s)" % (name, mask.device))
    return mask.to(torch.uint8).contiguous()


def _mesh_components_workspace(n_faces, n_vertices, device):
    return torch.empty(_lib().ngp_mesh_components_bytes(n_faces, n_vertices), device=device, dtype=torch.uint8)


def mesh_components_label(faces, n_vertices, max_rounds=None):
    """Labels of the pieces of a mesh (csrc/mesh_components.hip): faces int32 [T,3] -> (vertex_component int32 [V], face_component int32
    [T], counts int32 [3] = {components, bad faces, unused vertices} ON THE DEVICE, rounds).  rounds: the hook passes of the union-find
    up to and including the first that changed nothing; the flags are read once per MESH_COMPONENTS_BATCH rounds.  More than max_rounds
    (default V, which the scheme guarantees) raises RuntimeError."""
    n_faces, n_vertices = _mesh_faces(faces, n_vertices)
    dev = faces.device
    if n_faces == 0 or n_vertices == 0:                # nothing to join: every face is bad (V = 0) or every vertex unused (T = 0)
        counts = torch.tensor([0, n_faces, n_vertices], device=dev, dtype=torch.int32)
        return (torch.full((n_vertices,), -1, device=dev, dtype=torch.int32), torch.full((n_faces,), -1, device=dev, dtype=torch.int32),
                counts, 0)
    cap = n_vertices if max_rounds is None else int(max_rounds)
    parent = torch.arange(n_vertices, device=dev, dtype=torch.int32)
    rounds = 0
    while True:
        changed = torch.zeros(MESH_COMPONENTS_BATCH, device=dev, dtype=torch.int32)
        check(_lib().ngp_mesh_components_rounds(_ptr(faces), n_faces, n_vertices, _ptr(parent), _ptr(changed), MESH_COMPONENTS_BATCH,
                                                _stream()), "ngp_mesh_components_rounds")
        flags = changed.tolist()
        if 0 in flags:
            rounds += flags.index(0) + 1
            break
        rounds += MESH_COMPONENTS_BATCH
        if rounds >= cap:
            raise RuntimeError("the component labelling did not settle within %d rounds (the scheme guarantees V = %d)" % (cap, n_vertices))
    if rounds > cap:
        raise RuntimeError("the component labelling took %d rounds, more than the cap %d" % (rounds, cap))
    workspace = _mesh_components_workspace(n_faces, n_vertices, dev)
    vertex_component = torch.empty(n_vertices, device=dev, dtype=torch.int32)
    face_component = torch.empty(n_faces, device=dev, dtype=torch.int32)
    counts = torch.empty(3, device=dev, dtype=torch.int32)
    check(_lib().ngp_mesh_components_label(_ptr(faces), n_faces, n_vertices, _ptr(parent), _ptr(workspace), _ptr(vertex_component),
                                           _ptr(face_component), _ptr(counts), _stream()), "ngp_mesh_components_label")
    return vertex_component, face_component, counts, rounds


def _mesh_labels(faces, n_vertices, vertex_component, face_component):
    n_faces, n_vertices = _mesh_faces(faces, n_vertices)
    _dev(vertex_component, torch.int32, "vertex_component"); _dev(face_component, torch.int32, "face_component")
    if tuple(vertex_component.shape) != (n_vertices,) or tuple(face_component.shape) != (n_faces,):
        raise ValueError("vertex_component must be [V] and face_component [T]")
    return n_faces, n_vertices


def mesh_components_table(faces, n_vertices, vertex_component, face_component, n_components):
    """The integer columns of the per-component table -> int32 [C,6] (MESH_TABLE_COLUMNS).  The 3 T edge keys are sorted by torch.sort."""
    n_faces, n_vertices = _mesh_labels(faces, n_vertices, vertex_component, face_component)
    n_components = int(n_components)
    table = torch.empty(n_components, 6, device=faces.device, dtype=torch.int32)
    if n_components == 0:
        return table
    keys = torch.empty(3 * n_faces, device=faces.device, dtype=torch.int64)
    check(_lib().ngp_mesh_components_edge_keys(_ptr(faces), n_faces, n_vertices, _ptr(keys), _stream()), "ngp_mesh_components_edge_keys")
    keys = torch.sort(keys).values
    check(_lib().ngp_mesh_components_table(n_faces, n_vertices, _ptr(vertex_component), _ptr(face_component), _ptr(keys), n_components,
                                           _ptr(table), _stream()), "ngp_mesh_components_table")
    return table


def mesh_components_measure(vertices, faces, face_component, face_counts, n_bad):
    """Area f64 [C], signed volume f64 [C] and the box lo, hi f32 [C,3] of every component, summed in an order the input fixes.
    face_counts int32 [C]: the table's faces column; n_bad: the number of bad faces (they sort first)."""
    n_faces, n_vertices = _mesh_arrays(vertices, faces)
    _dev(face_counts, torch.int32, "face_counts"); _dev(face_component, torch.int32, "face_component")
    if tuple(face_component.shape) != (n_faces,):
        raise ValueError("face_component must be [T]")
    dev, n_components = faces.device, int(face_counts.shape[0])
    area = torch.empty(n_components, device=dev, dtype=torch.float64)
    volume = torch.empty(n_components, device=dev, dtype=torch.float64)
    lo = torch.empty(n_components, 3, device=dev, dtype=torch.float32)
    hi = torch.empty(n_components, 3, device=dev, dtype=torch.float32)
    if n_components == 0:
        return area, volume, lo, hi
    order = torch.sort(face_component, stable=True).indices                      # by (component, face index): bad faces (-1) first
    zero = torch.zeros(1, device=dev, dtype=torch.int32)
    face_start = torch.cat([zero, torch.cumsum(face_counts, 0, dtype=torch.int32)]) + int(n_bad)
    block_start = torch.cat([zero, torch.cumsum((face_counts + 63) // 64, 0, dtype=torch.int32)])
    partials = torch.empty(_lib().ngp_mesh_components_partial_bytes(n_faces, n_components) // 8, device=dev, dtype=torch.float64)
    check(_lib().ngp_mesh_components_measure(_ptr(vertices), _ptr(faces), _ptr(order), n_faces, n_vertices, _ptr(face_start),
                                             _ptr(block_start), n_components, _ptr(partials), _ptr(area), _ptr(volume), _ptr(lo), _ptr(hi),
                                             _stream()), "ngp_mesh_components_measure")
    return area, volume, lo, hi


def mesh_select(vertices, normals, faces, vertex_component, face_component, keep):
    """The sub-mesh of the components keep (uint8 / bool [C], on the device) marks -> (vertices, normals or None, faces, vertex_map int32
    [V], face_map int32 [T]): kept rows in their original relative order, faces re-indexed, the maps -1 for what is dropped.  One host
    read (the two sizes); an empty selection launches no emit."""
    _mesh_arrays(vertices)
    n_faces, n_vertices = _mesh_labels(faces, vertices.shape[0], vertex_component, face_component)
    if normals is not None:
        _dev(normals, torch.float32, "normals")
        if tuple(normals.shape) != tuple(vertices.shape):
            raise ValueError("normals must be [V,3] like the vertices")
    keep = _mesh_mask(keep, "keep")
    dev, n_components = faces.device, int(keep.shape[0])
    vertex_map = torch.full((n_vertices,), -1, device=dev, dtype=torch.int32)
    face_map = torch.full((n_faces,), -1, device=dev, dtype=torch.int32)
    n_v = n_f = 0
    if n_components and n_faces and n_vertices:
        counts = torch.empty(2, device=dev, dtype=torch.int32)
        workspace = _mesh_components_workspace(n_faces, n_vertices, dev)
        check(_lib().ngp_mesh_select_count(n_faces, n_vertices, _ptr(vertex_component), _ptr(face_component), _ptr(keep), n_components,
                                           _ptr(workspace), _ptr(vertex_map), _ptr(face_map), _ptr(counts), _stream()),
              "ngp_mesh_select_count")
        n_v, n_f = counts.tolist()                                               # the one synchronisation: the outputs' sizes
    out_v = torch.empty(n_v, 3, device=dev, dtype=torch.float32)
    out_n = torch.empty(n_v, 3, device=dev, dtype=torch.float32) if normals is not None else None
    out_f = torch.empty(n_f, 3, device=dev, dtype=torch.int32)
    if n_v and n_f:                                                              # a kept component has both; nothing kept: no launch
        check(_lib().ngp_mesh_select_emit(_ptr(vertices), _ptr(normals), _ptr(faces), n_faces, n_vertices, _ptr(vertex_map), _ptr(face_map),
                                          n_v, n_f, _ptr(out_v), _ptr(out_n), _ptr(out_f), _stream()), "ngp_mesh_select_emit")
    return out_v, out_n, out_f, vertex_map, face_map


# ---------------------------------------------------------------------------------------------------- mesh simplification
MESH_SIMPLIFY_MAX_CELLS = 2**21       # per axis: the cell key fits 63 bits; 2^21 on all three axes is refused (its last key is INT64_MAX)
MESH_SIMPLIFY_COUNTS = ("clusters", "vertices", "faces", "bad_vertices", "bad_faces")


def _mesh_simplify_grid(lo, h, n):
    """-> the four host arrays of the C ABI (lo, inv_h = 1 / h in f32, h, n); the contract's conditions are checked here."""
    lo, h = np.asarray(lo, np.float32).reshape(-1), np.asarray(h, np.float32).reshape(-1)
    n = [int(x) for x in n]
    if lo.shape != (3,) or h.shape != (3,) or len(n) != 3:
        raise ValueError("lo, h and n must hold three values each")
    inv_h = np.float32(1.0) / h if (h > 0).all() else np.zeros(3, np.float32)
    if not (np.isfinite(lo).all() and np.isfinite(h).all() and (h > 0).all() and np.isfinite(inv_h).all() and (inv_h > 0).all()):
        raise ValueError("lo must be finite and h positive and finite with a finite positive 1 / h in float32, got lo=%r h=%r" % (lo.tolist(), h.tolist()))
    if not all(1 <= x <= MESH_SIMPLIFY_MAX_CELLS for x in n) or n[0] * n[1] * n[2] >= 2**63:
        raise ValueError("every n must be in 1..2^21 (cells per axis) and their product below 2^63, got %r" % (n,))
    return (ctypes.c_float * 3)(*lo.tolist()), (ctypes.c_float * 3)(*inv_h.tolist()), (ctypes.c_float * 3)(*h.tolist()), (ctypes.c_int32 * 3)(*n)


def mesh_simplify_count(vertices, faces, lo, h, n):
    """The count phase of the simplification (csrc/mesh_simplify.hip) on the grid lo + [0, n) h: cell keys, their stable torch.sort,
    the cluster numbering, surviving faces and the two maps -> a SimpleNamespace with vertex_map int32 [V], face_map int32 [T], counts
    int32 [5] (MESH_SIMPLIFY_COUNTS) ON THE DEVICE, and what mesh_simplify_emit needs.  No quadric is formed, nothing is read back.
    V >= 1; T = 0 is allowed."""
    n_faces, n_vertices = _mesh_arrays(vertices, faces)
    if n_vertices < 1:
        raise ValueError("mesh_simplify_count needs at least one vertex")
    grid = _mesh_simplify_grid(lo, h, n)
    dev = vertices.device
    keys = torch.empty(n_vertices, device=dev, dtype=torch.int64)
    counts = torch.empty(5, device=dev, dtype=torch.int32)
    check(_lib().ngp_mesh_simplify_keys(_ptr(vertices), n_vertices, *grid, _ptr(keys), _ptr(counts), _stream()), "ngp_mesh_simplify_keys")
    keys, order = torch.sort(keys, stable=True)
    workspace = torch.empty(_lib().ngp_mesh_simplify_bytes(n_faces, n_vertices), device=dev, dtype=torch.uint8)
    st = SimpleNamespace(grid=grid, vertex_keys=keys, vertex_order=order, counts=counts,
                         vertex_cluster=torch.empty(n_vertices, device=dev, dtype=torch.int32),
                         cluster_out=torch.empty(n_vertices, device=dev, dtype=torch.int32),
                         vertex_map=torch.empty(n_vertices, device=dev, dtype=torch.int32),
                         face_map=torch.empty(n_faces, device=dev, dtype=torch.int32))
    check(_lib().ngp_mesh_simplify_count(_ptr(faces), n_faces, n_vertices, _ptr(keys), _ptr(order), _ptr(workspace), _ptr(st.vertex_cluster),
                                         _ptr(st.cluster_out), _ptr(st.vertex_map), _ptr(st.face_map), _ptr(counts), _stream()),
          "ngp_mesh_simplify_count")
    return st


def mesh_simplify_emit(vertices, faces, state, n_clusters, n_out_vertices, n_out_faces, regularization=1e-3, normals=True):
    """The second phase, after mesh_simplify_count on the same mesh (state) and with the host's copies of its counts: incidence keys,
    their stable torch.sort, the per-cluster sums and solves, the surviving faces -> (vertices f32 [V',3], normals f32 [V',3] or None,
    faces int32 [T',3]).  Nothing survives: empty tensors, no launch."""
    regularization = float(regularization)
    if not regularization > 0.0:
        raise ValueError("regularization must be positive (inf: the cluster mean), got %r" % (regularization,))
    n_faces, n_vertices = _mesh_arrays(vertices, faces)
    dev = vertices.device
    out_v = torch.empty(n_out_vertices, 3, device=dev, dtype=torch.float32)
    out_n = torch.empty(n_out_vertices, 3, device=dev, dtype=torch.float32) if normals else None
    out_f = torch.empty(n_out_faces, 3, device=dev, dtype=torch.int32)
    if n_out_vertices == 0 or n_out_faces == 0:
        return out_v, out_n, out_f
    if 3 * n_faces >= 2**31:
        raise ValueError("the mesh has %d faces; the simplification's incidence list holds at most 2^31 - 1 corners: simplify it in parts" % n_faces)
    keys = torch.empty(3 * n_faces, device=dev, dtype=torch.int64)
    check(_lib().ngp_mesh_simplify_incidence_keys(_ptr(vertices), _ptr(faces), n_faces, n_vertices, _ptr(state.vertex_cluster), _ptr(keys),
                                                  _stream()), "ngp_mesh_simplify_incidence_keys")
    keys, order = torch.sort(keys, stable=True)
    runs = torch.empty(_lib().ngp_mesh_simplify_runs_bytes(n_clusters, n_out_vertices) // 4, device=dev, dtype=torch.int32)
    check(_lib().ngp_mesh_simplify_emit(_ptr(vertices), _ptr(faces), n_faces, n_vertices, *state.grid, _ptr(state.vertex_keys),
                                        _ptr(state.vertex_order), _ptr(keys), _ptr(order), _ptr(state.vertex_cluster),
                                        _ptr(state.cluster_out), _ptr(state.vertex_map), _ptr(state.face_map), int(n_clusters),
                                        int(n_out_vertices), int(n_out_faces), regularization, _ptr(runs), _ptr(out_v), _ptr(out_n),
                                        _ptr(out_f), _stream()), "ngp_mesh_simplify_emit")
    return out_v, out_n, out_f


# ---------------------------------------------------------------------------------------------------- mesh smoothing
MESH_ADJACENCY_COUNTS = ("edges", "bad_faces", "bad_vertices", "boundary_vertices")
MESH_SMOOTH_MODES = {"fixed": _lib_mod._ABI.defines["NGP_MESH_SMOOTH_FIXED"], "curve": _lib_mod._ABI.defines["NGP_MESH_SMOOTH_CURVE"],
                     "free": _lib_mod._ABI.defines["NGP_MESH_SMOOTH_FREE"]}
MESH_FLAG_BOUNDARY, MESH_FLAG_NONMANIFOLD, MESH_FLAG_UNUSED, MESH_FLAG_BAD = 1, 2, 4, 8


def _mesh_smooth_sizes(vertices, faces):
    n_faces, n_vertices = _mesh_arrays(vertices, faces)
    if 6 * n_faces >= 2**31:
        raise ValueError("the mesh has %d faces; the adjacency's key list holds at most 2^31 - 1 directed edges" % n_faces)
    return n_faces, n_vertices


def mesh_adjacency(vertices, faces):
    """The vertex adjacency of a mesh as CSR, built on the device (csrc/mesh_smooth.hip): six directed keys per face, their torch.sort,
    runs, rows -> (row_start int32 [V + 1], neighbours int32 [6 T], multiplicity uint8 [6 T], vertex_flags uint8 [V], counts int32 [4]
    (MESH_ADJACENCY_COUNTS) ON THE DEVICE).  Only the first counts[0] slots of neighbours and multiplicity are written; nothing is read
    back.  V = 0 or T = 0: no launch (every face bad, every vertex unused)."""
    n_faces, n_vertices = _mesh_smooth_sizes(vertices, faces)
    dev = vertices.device
    row_start = torch.zeros(n_vertices + 1, device=dev, dtype=torch.int32)
    neighbours = torch.empty(6 * n_faces, device=dev, dtype=torch.int32)
    multiplicity = torch.empty(6 * n_faces, device=dev, dtype=torch.uint8)
    if n_faces == 0 or n_vertices == 0:
        bad = ~torch.isfinite(vertices).all(1)
        flags = MESH_FLAG_UNUSED + MESH_FLAG_BAD * bad.to(torch.uint8)
        counts = torch.tensor([0, n_faces, 0, 0], device=dev, dtype=torch.int32)
        counts[2] = bad.sum()
        return row_start, neighbours, multiplicity, flags, counts
    keys = torch.empty(6 * n_faces, device=dev, dtype=torch.int64)
    counts = torch.empty(4, device=dev, dtype=torch.int32)
    check(_lib().ngp_mesh_adjacency_keys(_ptr(faces), n_faces, n_vertices, _ptr(keys), _ptr(counts), _stream()), "ngp_mesh_adjacency_keys")
    keys = torch.sort(keys).values
    workspace = torch.empty(_lib().ngp_mesh_adjacency_bytes(n_faces), device=dev, dtype=torch.uint8)
    flags = torch.empty(n_vertices, device=dev, dtype=torch.uint8)
    check(_lib().ngp_mesh_adjacency_build(_ptr(vertices), n_faces, n_vertices, _ptr(keys), _ptr(workspace), _ptr(row_start), _ptr(neighbours),
                                          _ptr(multiplicity), _ptr(flags), _ptr(counts), _stream()), "ngp_mesh_adjacency_build")
    return row_start, neighbours, multiplicity, flags, counts


def mesh_smooth(vertices, row_start, neighbours, multiplicity, vertex_flags, iterations, lam, mu, boundary="fixed", fixed=None,
                max_move=None):
    """`iterations` Taubin iterations (a lambda pass, then a mu pass; mu = 0: lambda passes only) over the CSR of mesh_adjacency ->
    new positions f32 [V,3]; `vertices` is not written.  max_move: None or three floats >= 0 (inf: no bound on that axis), the bound
    on the displacement from `vertices`.  fixed: uint8 / bool [V] on the device or None.  No host read."""
    n_vertices = _mesh_arrays(vertices)[1]
    _dev(row_start, torch.int32, "row_start"); _dev(neighbours, torch.int32, "neighbours")
    _dev(multiplicity, torch.uint8, "multiplicity"); _dev(vertex_flags, torch.uint8, "vertex_flags")
    if tuple(row_start.shape) != (n_vertices + 1,) or tuple(vertex_flags.shape) != (n_vertices,) or neighbours.dim() != 1 \
            or multiplicity.shape != neighbours.shape:
        raise ValueError("row_start must be [V + 1], vertex_flags [V], neighbours and multiplicity [E] alike")
    if boundary not in MESH_SMOOTH_MODES:
        raise ValueError('boundary must be "fixed", "curve" or "free", got %r' % (boundary,))
    iterations, lam, mu = int(iterations), float(lam), float(mu)
    if iterations < 0 or not (np.isfinite(lam) and np.isfinite(mu)):
        raise ValueError("iterations must be >= 0 and lam, mu finite, got %r, %r, %r" % (iterations, lam, mu))
    move = np.full(3, np.inf, np.float32) if max_move is None else np.broadcast_to(np.asarray(max_move, np.float32).reshape(-1), (3,))
    if not (move >= 0).all():
        raise ValueError("max_move must be >= 0 (inf: no bound), got %r" % (max_move,))
    if fixed is not None:
        fixed = _mesh_mask(fixed, "fixed")
        if tuple(fixed.shape) != (n_vertices,):
            raise ValueError("fixed must be [V]")
    x_a = vertices.clone()
    passes = iterations * (1 if mu == 0.0 else 2)
    if n_vertices == 0 or passes == 0 or neighbours.shape[0] == 0:          # no edge: every vertex is unused, nothing moves
        return x_a
    x_b = torch.empty_like(x_a)
    check(_lib().ngp_mesh_smooth(_ptr(x_a), _ptr(x_b), _ptr(vertices), _ptr(row_start), _ptr(neighbours), _ptr(multiplicity),
                                 _ptr(vertex_flags), _ptr(fixed), n_vertices, int(neighbours.shape[0]), iterations, lam, mu,
                                 MESH_SMOOTH_MODES[boundary], (ctypes.c_float * 3)(*move.tolist()), _stream()), "ngp_mesh_smooth")
    return x_a if passes % 2 == 0 else x_b


def mesh_vertex_normals(vertices, faces):
    """Area-weighted vertex normals f32 [V,3] (csrc/mesh_smooth.hip): the f64 sum of the area vectors of a vertex's good faces in the
    order of the stably sorted incidence list, normalised; 0 where the sum is 0 or not finite.  No host read."""
    n_faces, n_vertices = _mesh_smooth_sizes(vertices, faces)
    dev = vertices.device
    normals = torch.zeros(n_vertices, 3, device=dev, dtype=torch.float32)
    if n_faces == 0 or n_vertices == 0:
        return normals
    keys = torch.empty(3 * n_faces, device=dev, dtype=torch.int64)
    check(_lib().ngp_mesh_vertex_normals_keys(_ptr(faces), n_faces, n_vertices, _ptr(keys), _stream()), "ngp_mesh_vertex_normals_keys")
    keys, order = torch.sort(keys, stable=True)
    check(_lib().ngp_mesh_vertex_normals(_ptr(vertices), _ptr(faces), n_faces, n_vertices, _ptr(keys), _ptr(order), _ptr(normals),
                                         _stream()), "ngp_mesh_vertex_normals")
    return normals


# ---------------------------------------------------------------------------------------------------- vertex colours
MESH_COLOR_MODES = {"blend": _lib_mod._ABI.defines["NGP_MESH_COLOR_BLEND"], "best": _lib_mod._ABI.defines["NGP_MESH_COLOR_BEST"]}
MESH_COLOR_PAIR_BYTES = 44              # per (vertex, camera) pair of a chunk: the segment 24, the sample 8, weight, cos and t 4 each
MESH_COLOR_UNCOLOURED = 255             # `filled` of a vertex that has no colour


def mesh_color_project(vertices, normals, K, c2w, img_wh, eps, cos_min=0.1, near=1e-6, two_sided=False):
    """One chunk of cameras against every vertex (csrc/mesh_color.hip): vertices, normals f32 [V,3], K f32 [3,3] or [N,3,3], c2w f32
    [N,3,4], eps f32 [1] ON THE DEVICE -> (rays_o [V N,3], rays_d [V N,3], sample [V N,2], weight [V N], cosv [V N]), pair j V + v.  A
    rejected pair has weight 0 and a zero ray.  V >= 1, N >= 1, V N < 2^31."""
    n_vertices = _mesh_arrays(vertices)[1]
    for t, name in ((normals, "normals"), (K, "K"), (c2w, "c2w"), (eps, "eps")):
        _dev(t, torch.float32, name)
    if tuple(normals.shape) != tuple(vertices.shape):
        raise ValueError("normals must be [V,3] like the vertices, got %s" % (tuple(normals.shape),))
    if c2w.dim() != 3 or tuple(c2w.shape[1:]) != (3, 4) or tuple(K.shape) not in ((3, 3), (c2w.shape[0], 3, 3)) or eps.numel() != 1:
        raise ValueError("c2w must be [N,3,4], K [3,3] or [N,3,3] and eps one element, got %s, %s, %s"
                         % (tuple(c2w.shape), tuple(K.shape), tuple(eps.shape)))
    n_cameras, (w, h) = int(c2w.shape[0]), (int(img_wh[0]), int(img_wh[1]))
    pairs = n_vertices * n_cameras
    if n_vertices < 1 or n_cameras < 1 or pairs >= 2**31 or w < 1 or h < 1:
        raise ValueError("need V >= 1, N >= 1, V N < 2^31 and a positive image size, got V %d, N %d, (W, H) (%d, %d)" % (n_vertices, n_cameras, w, h))
    if not float(cos_min) >= 0.0 or not float(near) >= 0.0:
        raise ValueError("cos_min and near must be >= 0, got %r and %r" % (cos_min, near))
    f32 = dict(device=vertices.device, dtype=torch.float32)
    rays_o, rays_d, sample = torch.empty(pairs, 3, **f32), torch.empty(pairs, 3, **f32), torch.empty(pairs, 2, **f32)
    weight, cosv = torch.empty(pairs, **f32), torch.empty(pairs, **f32)
    check(_lib().ngp_mesh_color_project(_ptr(vertices), _ptr(normals), n_vertices, _ptr(K), int(K.dim() == 3), _ptr(c2w), n_cameras, w, h,
                                        _ptr(eps), float(cos_min), float(near), int(bool(two_sided)), _ptr(rays_o), _ptr(rays_d),
                                        _ptr(sample), _ptr(weight), _ptr(cosv), _stream()), "ngp_mesh_color_project")
    return rays_o, rays_d, sample, weight, cosv


def mesh_color_accumulate(images, sample, weight, cosv, t, accum, views, best_cos=None, mode="blend"):
    """Adds one chunk into accum f64 [V,4] and views int32 [V] in place (best_cos f32 [V] too, mode "best"): images f32 [N,H,W,C >= 3] of
    the chunk, sample / weight / cosv of mesh_color_project, t [V N] of the any-hit ray cast over its segments."""
    if mode not in MESH_COLOR_MODES:
        raise ValueError('mode must be "blend" or "best", got %r' % (mode,))
    _dev(images, torch.float32, "images"); _dev(accum, torch.float64, "accum"); _dev(views, torch.int32, "views")
    for x, name in ((sample, "sample"), (weight, "weight"), (cosv, "cosv"), (t, "t")):
        _dev(x, torch.float32, name)
    if images.dim() != 4 or images.shape[3] < 3 or images.shape[0] < 1:
        raise ValueError("images must be [N,H,W,C] with C >= 3, got %s" % (tuple(images.shape),))
    n_cameras, h, w, c = (int(x) for x in images.shape)
    n_vertices = int(views.shape[0])
    pairs = n_vertices * n_cameras
    if tuple(accum.shape) != (n_vertices, 4) or views.dim() != 1 or n_vertices < 1 or pairs >= 2**31 \
            or any(x.numel() != k * pairs for x, k in ((sample, 2), (weight, 1), (cosv, 1), (t, 1))):
        raise ValueError("accum must be [V,4], views [V] and the per-pair arrays those of V x %d pairs" % n_cameras)
    if mode == "best":
        if best_cos is None or tuple(best_cos.shape) != (n_vertices,):
            raise ValueError('mode "best" needs best_cos f32 [V]')
        _dev(best_cos, torch.float32, "best_cos")
    check(_lib().ngp_mesh_color_accumulate(_ptr(images), n_cameras, h, w, c, n_vertices, _ptr(sample), _ptr(weight), _ptr(cosv), _ptr(t),
                                           MESH_COLOR_MODES[mode], _ptr(accum), _ptr(views), _ptr(best_cos if mode == "best" else None),
                                           _stream()), "ngp_mesh_color_accumulate")
    _touched(accum, views, best_cos if mode == "best" else None)


def mesh_color_finish(accum, views):
    """accum f64 [V,4], views int32 [V] -> (colors f32 [V,3], weight f32 [V], filled uint8 [V]: 0 where views > 0, else 255)."""
    _dev(accum, torch.float64, "accum"); _dev(views, torch.int32, "views")
    n_vertices = int(views.shape[0])
    if tuple(accum.shape) != (n_vertices, 4) or views.dim() != 1:
        raise ValueError("accum must be [V,4] and views [V]")
    dev = accum.device
    colors = torch.zeros(n_vertices, 3, device=dev, dtype=torch.float32)
    weight = torch.zeros(n_vertices, device=dev, dtype=torch.float32)
    filled = torch.full((n_vertices,), MESH_COLOR_UNCOLOURED, device=dev, dtype=torch.uint8)
    if n_vertices:
        check(_lib().ngp_mesh_color_finish(_ptr(accum), _ptr(views), n_vertices, _ptr(colors), _ptr(weight), _ptr(filled), _stream()),
              "ngp_mesh_color_finish")
    return colors, weight, filled


def mesh_color_fill(colors, filled, row_start, neighbours, rounds):
    """`rounds` Jacobi rounds (0 .. 254) over the CSR of mesh_adjacency: colors f32 [V,3] is updated IN PLACE, -> filled uint8 [V] after
    the last round (the input tensor itself for rounds = 0).  No host read: every round is launched."""
    _dev(colors, torch.float32, "colors"); _dev(filled, torch.uint8, "filled")
    _dev(row_start, torch.int32, "row_start"); _dev(neighbours, torch.int32, "neighbours")
    n_vertices = int(filled.shape[0])
    rounds = int(rounds)
    if tuple(colors.shape) != (n_vertices, 3) or tuple(row_start.shape) != (n_vertices + 1,) or neighbours.dim() != 1:
        raise ValueError("colors must be [V,3], filled [V], row_start [V + 1] and neighbours [E]")
    if not 0 <= rounds < MESH_COLOR_UNCOLOURED:
        raise ValueError("rounds must be in 0..254, got %r" % (rounds,))
    if n_vertices == 0 or neighbours.shape[0] == 0:
        return filled
    other = torch.empty_like(filled) if rounds else None
    for r in range(1, rounds + 1):
        check(_lib().ngp_mesh_color_fill(_ptr(colors), _ptr(filled), _ptr(other), _ptr(row_start), _ptr(neighbours), n_vertices,
                                         int(neighbours.shape[0]), r, _stream()), "ngp_mesh_color_fill")
        filled, other = other, filled
    _touched(colors)
    return filled


# ---------------------------------------------------------------------------------------------------- surface rendering
def _surface_inputs(sdf, cosv, rgbs, aux, deltas, ts, rays_a, inv_s):
    _dev(sdf, torch.float32, "sdf"); _dev(cosv, torch.float32, "cosv"); _dev(rgbs, torch.float32, "rgbs")
    _dev(deltas, torch.float32, "deltas"); _dev(ts, torch.float32, "ts"); _dev(rays_a, torch.int32, "rays_a")
    _dev(inv_s, torch.float32, "inv_s")
    S = sdf.numel()
    if sdf.dim() != 1 or cosv.shape != sdf.shape or deltas.shape != sdf.shape or ts.shape != sdf.shape or tuple(rgbs.shape) != (S, 3):
        raise ValueError("sdf, cosv, deltas, ts must be [S] and rgbs [S, 3]; got %s %s %s %s %s"
                         % tuple(tuple(t.shape) for t in (sdf, cosv, deltas, ts, rgbs)))
    if aux is not None:
        _dev(aux, torch.float32, "aux")
        if tuple(aux.shape) != (S, 3):
            raise ValueError("aux must be [S, 3], got %s" % (tuple(aux.shape),))
    if rays_a.dim() != 2 or rays_a.shape[1] != 3:
        raise ValueError("rays_a must be [n_rays, 3], got %s" % (tuple(rays_a.shape),))
    if inv_s.numel() != 1:
        raise ValueError("inv_s must hold one float (it is read on the device), got %d" % inv_s.numel())
    return S, rays_a.shape[0]


def surface_composite_fwd(sdf, cosv, rgbs, deltas, ts, rays_a, inv_s, cos_anneal=1.0, T_threshold=1e-4, aux=None, bg=0.0):
    """ngp_surface_composite_fwd (csrc/surface.hip; contract in include/ngp_hip.h): the NeuS-opacity compositor.
    -> (total_samples [n] i32, opacity [n], depth [n], rgb [n,3], rgb_out [n,3] = rgb + bg (1 - opacity), aux_out [n,3] or None,
    ws [S], alphas [S])."""
    S, n = _surface_inputs(sdf, cosv, rgbs, aux, deltas, ts, rays_a, inv_s)
    dev = sdf.device
    total_samples = torch.empty(n, device=dev, dtype=torch.int32)
    opacity, depth = torch.empty(n, device=dev), torch.empty(n, device=dev)
    rgb, rgb_out = torch.empty(n, 3, device=dev), torch.empty(n, 3, device=dev)
    aux_out = torch.empty(n, 3, device=dev) if aux is not None else None
    ws, alphas = torch.empty(S, device=dev), torch.empty(S, device=dev)
    check(_lib().ngp_surface_composite_fwd(_ptr(sdf), _ptr(cosv), _ptr(rgbs), _ptr(aux), _ptr(deltas), _ptr(ts), _ptr(rays_a), _ptr(inv_s),
                                           float(cos_anneal), float(T_threshold), n, float(bg), _ptr(total_samples), _ptr(opacity),
                                           _ptr(depth), _ptr(rgb), _ptr(rgb_out), _ptr(aux_out), _ptr(ws), _ptr(alphas), _stream()),
          "ngp_surface_composite_fwd")
    return total_samples, opacity, depth, rgb, rgb_out, aux_out, ws, alphas


def surface_composite_bwd(dL_dopacity, dL_ddepth, dL_drgb, dL_daux, dL_dws, sdf, cosv, rgbs, deltas, ts, rays_a, inv_s, total_samples, alphas,
                          cos_anneal=1.0, aux=None, bg=0.0):
    """ngp_surface_composite_bwd: -> (d_sdf [S], d_cos [S], d_rgbs [S,3], d_aux [S,3] or None, d_inv_s [1]).  Every cotangent but dL_drgb
    may be None; dL_drgb is the gradient of rgb_out when bg != 0.  d_inv_s is summed without atomics: bit-reproducible."""
    S, n = _surface_inputs(sdf, cosv, rgbs, aux, deltas, ts, rays_a, inv_s)
    if dL_drgb is None:
        raise ValueError("dL_drgb is required")
    for name, t, shape in (("dL_dopacity", dL_dopacity, (n,)), ("dL_ddepth", dL_ddepth, (n,)), ("dL_drgb", dL_drgb, (n, 3)),
                           ("dL_daux", dL_daux, (n, 3)), ("dL_dws", dL_dws, (S,))):
        if t is not None:
            _dev(t, torch.float32, name)
            if tuple(t.shape) != shape:
                raise ValueError("%s must be %s, got %s" % (name, shape, tuple(t.shape)))
    if dL_daux is not None and aux is None:
        raise ValueError("dL_daux without aux")
    _dev(total_samples, torch.int32, "total_samples"); _dev(alphas, torch.float32, "alphas")
    if total_samples.numel() != n or alphas.numel() != S:
        raise ValueError("total_samples must be [n_rays] and alphas [S]")
    dev = sdf.device
    d_sdf, d_cos, d_rgbs = torch.empty(S, device=dev), torch.empty(S, device=dev), torch.empty(S, 3, device=dev)
    d_aux = torch.empty(S, 3, device=dev) if aux is not None else None
    d_inv_s = torch.zeros(1, device=dev)
    workspace = torch.empty(max(n, 1), device=dev)
    check(_lib().ngp_surface_composite_bwd(_ptr(dL_dopacity), _ptr(dL_ddepth), _ptr(dL_drgb), _ptr(dL_daux), _ptr(dL_dws), _ptr(sdf),
                                           _ptr(cosv), _ptr(rgbs), _ptr(aux), _ptr(deltas), _ptr(ts), _ptr(rays_a), _ptr(inv_s),
                                           float(cos_anneal), n, float(bg), _ptr(total_samples), _ptr(alphas), _ptr(d_sdf), _ptr(d_cos),
                                           _ptr(d_rgbs), _ptr(d_aux), _ptr(d_inv_s), _ptr(workspace), _stream()),
          "ngp_surface_composite_bwd")
    return d_sdf, d_cos, d_rgbs, d_aux, d_inv_s


# ---------------------------------------------------------------------------------------------------- importance resampling
def resample_rays(ws, deltas, ts, rays_a, rays_o, rays_d, noise, K, floor=0.0):
    """ngp_resample_count -> _scan -> (one D2H read of the total, like march_train) -> _write (csrc/resample.hip; contract in
    include/ngp_hip.h): K stratified inverse-CDF draws per ray cut the marched sections where the weight ws is.
    ws, deltas, ts [S]; rays_a [n,3] i32 (ray index, start, count); rays_o, rays_d [n_orig,3] and noise [n_orig] in [0, 1), indexed
    by the ray index.  -> (rays_a' [n,3], xyzs [S',3], dirs [S',3], deltas [S'], ts [S'], parent [S'] i32, total): the same rows and
    ray indices, children in ascending t, parent = the index of the coarse sample a child was cut from.  Nothing is differentiable."""
    for name, t in (("ws", ws), ("deltas", deltas), ("ts", ts), ("rays_o", rays_o), ("rays_d", rays_d), ("noise", noise)):
        _dev(t, torch.float32, name)
    _dev(rays_a, torch.int32, "rays_a")
    S, K = ws.numel(), int(K)
    if ws.dim() != 1 or deltas.shape != ws.shape or ts.shape != ws.shape:
        raise ValueError("ws, deltas, ts must be [S]; got %s %s %s" % (tuple(ws.shape), tuple(deltas.shape), tuple(ts.shape)))
    if rays_a.dim() != 2 or rays_a.shape[1] != 3:
        raise ValueError("rays_a must be [n_rays, 3], got %s" % (tuple(rays_a.shape),))
    n, n_orig = rays_a.shape[0], rays_o.shape[0]
    if rays_o.dim() != 2 or rays_o.shape[1] != 3 or rays_d.shape != rays_o.shape or tuple(noise.shape) != (n_orig,):
        raise ValueError("rays_o, rays_d must be [n_orig, 3] and noise [n_orig]; got %s %s %s"
                         % (tuple(rays_o.shape), tuple(rays_d.shape), tuple(noise.shape)))
    if K < 1:
        raise ValueError("K must be at least 1, got %d" % K)
    if not float(floor) >= 0.0:
        raise ValueError("floor must be >= 0, got %r" % (floor,))
    if S + n * K >= 2**31:
        raise ValueError("S + n_rays K = %d does not fit the int32 sample index" % (S + n * K))
    dev = ws.device
    rays_a_out = torch.empty(n, 3, device=dev, dtype=torch.int32)
    total = torch.zeros(2, device=dev, dtype=torch.int32)
    empty = lambda m, dt=torch.float32: torch.empty(m, device=dev, dtype=dt)
    if n == 0:
        return rays_a_out, empty((0, 3)), empty((0, 3)), empty(0), empty(0), empty(0, torch.int32), total[0]
    if n_orig < 1:
        raise ValueError("rays_a has rows but rays_o is empty")
    L, st = _lib(), _stream()
    cdf, stage_t, stage_j, counts = empty(S), empty(n * K), empty(n * K, torch.int32), empty(n, torch.int32)
    check(L.ngp_resample_count(_ptr(ws), _ptr(deltas), _ptr(ts), _ptr(rays_a), _ptr(noise), n, n_orig, S, K, float(floor), _ptr(cdf),
                               _ptr(stage_t), _ptr(stage_j), _ptr(counts), _ptr(total), st), "ngp_resample_count")
    check(L.ngp_resample_scan(_ptr(counts), _ptr(rays_a), n, _ptr(rays_a_out), _ptr(total), st), "ngp_resample_scan")
    S_out, bad = (int(v) for v in total.tolist())
    if bad:
        raise ValueError("rays_a has a row outside the buffers (ray index outside [0, %d), or start / count outside [0, %d])" % (n_orig, S))
    xyzs, dirs, deltas_out, ts_out, parent = empty((S_out, 3)), empty((S_out, 3)), empty(S_out), empty(S_out), empty(S_out, torch.int32)
    if S_out > 0:
        check(L.ngp_resample_write(_ptr(rays_o), _ptr(rays_d), _ptr(deltas), _ptr(ts), _ptr(rays_a), _ptr(rays_a_out), _ptr(stage_t),
                                   _ptr(stage_j), n, n_orig, S, K, _ptr(xyzs), _ptr(dirs), _ptr(deltas_out), _ptr(ts_out), _ptr(parent),
                                   st), "ngp_resample_write")
    return rays_a_out, xyzs, dirs, deltas_out, ts_out, parent, total[0]


# ---------------------------------------------------------------------------------------------------- sphere tracing
SDF_DT_MIN = float(np.float32(1.7320508075688772 / 1024))
SDF_TRACE_DEFAULTS = dict(eps=1e-4, step_scale=1.0, min_step=SDF_DT_MIN, n_refine=8, max_evals=256)


def sdf_pack(layers):
    """The fp32 weight pack of ngp_sdf_eval / ngp_sdf_trace from the geometry MLP's linear layers (objects with .weight [out, in] and
    .bias [out]): W0 | b0 | (Wi | bi).. | w_out | b_out, of the last layer row 0 only.  A fresh tensor: a copy of the parameters."""
    layers = list(layers)
    if len(layers) < 2:
        raise ValueError("sdf_pack needs at least one hidden layer and the output layer")
    parts = []
    for lin in layers[:-1]:
        parts += [lin.weight.detach().float().reshape(-1), lin.bias.detach().float().reshape(-1)]
    parts += [layers[-1].weight.detach().float()[0].reshape(-1), layers[-1].bias.detach().float()[:1]]
    return torch.cat(parts).contiguous()


def sdf_pack_size(n_levels, width, depth):
    return width * (3 + 2 * n_levels) + width + (depth - 1) * (width * width + width) + width + 1


def _sdf_field_check(what, table, lv, wpack, width, depth):
    width, depth = int(width), int(depth)
    if lv.n_features != 2 or not 1 <= lv.n_levels <= 16:
        raise ValueError("%s needs a level table of 1..16 levels with 2 features, got %d x %d" % (what, lv.n_levels, lv.n_features))
    if width not in (16, 32, 64) or depth not in (1, 2):
        raise ValueError("%s supports width 16, 32 or 64 and depth 1 or 2, got width %d depth %d" % (what, width, depth))
    _dev(table, torch.float32, "hash_table"); _dev(wpack, torch.float32, "wpack")
    if table.numel() != lv.total_entries * 2:
        raise ValueError("%s: the table must hold %d floats, got %d" % (what, lv.total_entries * 2, table.numel()))
    if wpack.numel() != sdf_pack_size(lv.n_levels, width, depth):
        raise ValueError("%s: the pack of %d levels, width %d, depth %d holds %d floats, got %d"
                         % (what, lv.n_levels, width, depth, sdf_pack_size(lv.n_levels, width, depth), wpack.numel()))
    return width, depth


def sdf_eval(xyzs, table, lv, wpack, width, depth, scale, return_enc=False):
    """The SDF field's geometry value in one launch (ngp_sdf_eval; contract in include/ngp_hip.h, "sphere tracing"): world positions
    [n,3] -> f [n], plus the [n, 2 L] embedding with return_enc=True (bit for bit hash_fwd_f32 of the normalised positions)."""
    _dev(xyzs, torch.float32, "xyzs")
    n = xyzs.shape[0]
    if tuple(xyzs.shape) != (n, 3):
        raise ValueError("sdf_eval: xyzs must be [n, 3], got %s" % (tuple(xyzs.shape),))
    width, depth = _sdf_field_check("sdf_eval", table, lv, wpack, width, depth)
    f = torch.empty(n, device=xyzs.device, dtype=torch.float32)
    enc = torch.empty(n, 2 * lv.n_levels, device=xyzs.device, dtype=torch.float32) if return_enc else None
    check(_lib().ngp_sdf_eval(_ptr(xyzs), _ptr(table), ctypes.byref(lv), _ptr(wpack), width, depth, float(scale), n, _ptr(f), _ptr(enc),
                              _stream()), "ngp_sdf_eval")
    return (f, enc) if return_enc else f


def sdf_trace(rays_o, rays_d, density_bitfield, coarse, table, lv, wpack, width, depth, cascades, scale, grid_size, eps=1e-4,
              step_scale=1.0, min_step=SDF_DT_MIN, n_refine=8, max_evals=256, out=None, stats=None):
    """Sphere tracing in one launch (ngp_sdf_trace; the rule is the "sphere tracing" block of include/ngp_hip.h).  rays_o, rays_d [n,3]
    f32, directions unit vectors; density_bitfield uint8 [cascades * grid_size^3 / 8]; coarse: coarse_bitfield(...) or None.
    -> (status [n] i32: 0 MISS, 1 HIT, 2 INSIDE, 3 ABANDONED; t [n]; xyz [n,3]; n_eval [n] i32; f_last [n]); `out` = that tuple
    preallocated.  stats: None or a zeroed int64 [2] that receives (lane slots of the evaluation rounds, slots that evaluated)."""
    f32, i32, n = torch.float32, torch.int32, rays_o.shape[0]
    cascades, grid_size = int(cascades), int(grid_size)
    want = [(rays_o, "rays_o", f32, (n, 3)), (rays_d, "rays_d", f32, (n, 3)),
            (density_bitfield, "density_bitfield", torch.uint8, (cascades * grid_size**3 // 8,))]
    if coarse is not None:
        want.append((coarse, "coarse", i32, (cascades * grid_size**3 // 512 // 32,)))
    if out is not None:
        status, t, xyz, n_eval, f_last = out
        want += [(status, "out status", i32, (n,)), (t, "out t", f32, (n,)), (xyz, "out xyz", f32, (n, 3)), (n_eval, "out n_eval", i32, (n,)),
                 (f_last, "out f_last", f32, (n,))]
    if stats is not None:
        want.append((stats, "stats", torch.int64, (2,)))
    for x, name, dt, shape in want:
        if x.dtype != dt or tuple(x.shape) != shape:
            raise ValueError("sdf_trace: %s must be %s %s, got %s %s" % (name, dt, shape, x.dtype, tuple(x.shape)))
    for x, name, dt, _ in want:
        _dev(x, dt, name)
    width, depth = _sdf_field_check("sdf_trace", table, lv, wpack, width, depth)
    if out is None:
        dev = rays_o.device
        out = (torch.empty(n, device=dev, dtype=i32), torch.empty(n, device=dev), torch.empty(n, 3, device=dev),
               torch.empty(n, device=dev, dtype=i32), torch.empty(n, device=dev))
    status, t, xyz, n_eval, f_last = out
    check(_lib().ngp_sdf_trace(_ptr(rays_o), _ptr(rays_d), _ptr(density_bitfield), _ptr(coarse), _ptr(table), ctypes.byref(lv), _ptr(wpack),
                               width, depth, cascades, float(scale), grid_size, n, float(eps), float(step_scale), float(min_step),
                               int(n_refine), int(max_evals), _ptr(status), _ptr(t), _ptr(xyz), _ptr(n_eval), _ptr(f_last), _ptr(stats),
                               _stream()), "ngp_sdf_trace")
    _touched(*out)
    return out


def levels_to_numpy(lv):
    """(scale, resolution, map_size, offset) as numpy arrays -- for tests and for the module buffers."""
    L = lv.n_levels
    return (np.array(lv.scale[:L], dtype=np.float32), np.array(lv.resolution[:L], dtype=np.uint32),
            np.array(lv.map_size[:L], dtype=np.uint32), np.array(lv.offset[:L], dtype=np.uint32))
