"""Loader and renderer for exported deployment models (train.py --deployment): the reference's second program,
deployment/InstantNGP/taichi_ngp/taichi_ngp.py `run_inference`, on the HIP kernels.

A deployment model is a 4-level, 4-feature dense grid (base 32, max 128, log2_T 21: 2 794 024 entries) with a 16 -> 16 -> 16 density
network and a [SH16 | 16] -> 16 -> 3 colour network, one 128^3 occupancy cascade at scale 0.5.  It exists in two file formats, both
written by this package: `deployment.npy` (modules.utils.save_deployment_model) and a folder of `.bin` blobs
(ngp_hip.export.export_deployment_bins, fp32 or fp16).  `DeployedModel` reads either -- or takes a live NGP -- and renders images:

    m = DeployedModel.from_npy("deployment.npy")        # or .from_bins(folder) / .from_module(ngp_model)
    out = m.render(m.poses[20], res=(300, 600))          # {'rgb', 'opacity', 'depth', 'total_samples'}

Loading and validation are host-side numpy; shading and rendering need the GPU (there is no CPU path).  Rays are marched and
composited by the package's existing kernels; the shading between them is ngp_deploy_shade (csrc/deploy.hip), fp32 throughout.
render(..., mode="fused") does all of it per ray in one launch instead (ngp_deploy_render)."""
import os

import numpy as np
import torch

from . import ops
from .export import read_bin

BASE_RES, MAX_RES, LEVELS, FEATURES, LOG2_T = 32, 128, 4, 4, 21
GRID_SIZE, SCALE, CASCADES = 128, 0.5, 1
SIGMA_WEIGHTS, RGB_WEIGHTS = 16 * 16 + 16 * 16, 32 * 16 + 16 * 16
BITFIELD_BYTES = CASCADES * GRID_SIZE**3 // 8
DEPLOYMENT_CONFIG = dict(scale=SCALE, pos_encoder_type='hash', levels=LEVELS, feature_per_level=FEATURES, base_res=BASE_RES, max_res=MAX_RES,
                         log2_T=LOG2_T, xyz_net_width=16, rgb_net_width=16, rgb_net_depth=1)      # train.py --deployment
RENDER_CHUNK = 65536


def get_directions(res_w, res_h, camera_angle_x=0.5):
    """Camera-frame ray directions of a res_w x res_h image, [res_h * res_w, 3] f32 in row-major pixel order: pixel centres, each
    axis with a focal length of its own from the same angle (the formula of the reference's load_deployment_model)."""
    w, h = int(res_w), int(res_h)
    fx, fy = 0.5 * w / np.tan(0.5 * camera_angle_x), 0.5 * h / np.tan(0.5 * camera_angle_x)
    x, y = np.meshgrid(np.arange(w, dtype=np.float32) + 0.5, np.arange(h, dtype=np.float32) + 0.5, indexing='xy')
    return np.stack([(x - 0.5 * w) / fx, (y - 0.5 * h) / fy, np.ones_like(x)], -1).reshape(-1, 3).astype(np.float32)


def _floats(name, a):
    a = np.asarray(a)
    if a.dtype not in (np.float32, np.float16):
        raise ValueError("%s: dtype %s is not a deployment payload (float32 or float16)" % (name, a.dtype))
    return np.ascontiguousarray(a.reshape(-1).astype(np.float32))              # fp16 blobs are widened on load


class DeployedModel:
    """The arrays of one deployment model, validated; device copies are made on first use."""

    def __init__(self, hash_table, sigma_weights, rgb_weights, density_bitfield, poses=None, per_level_scale=None, device=None):
        self.levels = ops.make_levels(2**LOG2_T, LEVELS, BASE_RES, MAX_RES, FEATURES)
        self.log_b = float(np.log(MAX_RES / BASE_RES) / (LEVELS - 1))          # the level table's own per-level scale
        self.hash_table = _floats("hash table", hash_table)
        self.sigma_weights = _floats("sigma weights", sigma_weights)
        self.rgb_weights = _floats("rgb weights", rgb_weights)
        bits = np.ascontiguousarray(density_bitfield)
        if bits.dtype not in (np.uint8, np.uint32, np.int32):
            raise ValueError("density bitfield: dtype %s (uint8 bytes or uint32 words expected)" % bits.dtype)
        self.density_bitfield = bits.reshape(-1).view(np.uint8)
        want = int(self.levels.total_entries) * FEATURES
        if self.hash_table.size != want:
            raise ValueError("hash table has %d values, the 4-level table (base 32, max 128, 4 features) holds %d" % (self.hash_table.size, want))
        if self.sigma_weights.size != SIGMA_WEIGHTS:
            raise ValueError("sigma weights: %d values, the 16 -> 16 -> 16 network has %d" % (self.sigma_weights.size, SIGMA_WEIGHTS))
        if self.rgb_weights.size != RGB_WEIGHTS:
            raise ValueError("rgb weights: %d values, the 32 -> 16 -> 3 network (output padded to 16 rows) has %d"
                             % (self.rgb_weights.size, RGB_WEIGHTS))
        if self.density_bitfield.size != BITFIELD_BYTES:
            # the formats carry no scale: one 128^3 cascade, i.e. scale 0.5, is the only shape a deployment model has
            raise ValueError("density bitfield: %d bytes, one 128^3 cascade has %d" % (self.density_bitfield.size, BITFIELD_BYTES))
        if per_level_scale is not None and abs(float(per_level_scale) - self.log_b) > 1e-6 * self.log_b:
            raise ValueError("model.per_level_scale = %r, the level table is built with %r" % (float(per_level_scale), self.log_b))
        self.poses = None if poses is None else np.asarray(poses, np.float32).reshape(-1, 3, 4)
        self.device = torch.device(device) if device is not None else None
        self._dev = None
        self._coarse = None

    # ------------------------------------------------------------------------------------------ loaders
    @classmethod
    def from_npy(cls, path_or_dict, device=None):
        """`deployment.npy` of modules.utils.save_deployment_model (a path, or the dictionary itself)."""
        d = path_or_dict
        if isinstance(d, (str, os.PathLike)):
            if not os.path.isfile(d):
                raise ValueError("no deployment model at %s" % d)
            d = np.load(d, allow_pickle=True).item()
        keys = ('model.hash_encoder.params', 'model.xyz_encoder.params', 'model.rgb_net.params', 'model.density_bitfield',
                'model.per_level_scale')
        missing = [k for k in keys if k not in d]
        if missing:
            raise ValueError("deployment model lacks %s" % ", ".join(missing))
        return cls(d['model.hash_encoder.params'], d['model.xyz_encoder.params'], d['model.rgb_net.params'], d['model.density_bitfield'],
                   poses=d.get('poses'), per_level_scale=d['model.per_level_scale'], device=device)

    @classmethod
    def from_bins(cls, folder, device=None):
        """The blob folder of ngp_hip.export.export_deployment_bins / the reference's exporter (fp32 or fp16 payloads)."""
        folder = str(folder)
        arrays = {}
        for name in ("hash_embedding", "sigma_weights", "rgb_weights", "density_bitfield"):
            path = os.path.join(folder, name + ".bin")
            if not os.path.isfile(path):
                raise ValueError("blob folder %s lacks %s.bin" % (folder, name))
            arrays[name] = read_bin(path)
        pose = os.path.join(folder, "pose.bin")
        poses = _floats("pose", read_bin(pose)) if os.path.isfile(pose) else None
        if poses is not None and poses.size != 12:
            raise ValueError("pose.bin holds %d values, a 3x4 camera-to-world has 12" % poses.size)
        return cls(arrays["hash_embedding"], arrays["sigma_weights"], arrays["rgb_weights"], arrays["density_bitfield"], poses=poses,
                   device=device)

    @classmethod
    def from_module(cls, model, poses=None):
        """A live NGP built with train.py's --deployment configuration; any other architecture is refused."""
        enc = getattr(model, 'pos_encoder', None)
        lv = getattr(enc, 'levels_struct', None)
        ok = (getattr(model, 'pos_encoder_type', None) == 'hash' and lv is not None and not getattr(model, 'half_opt', False)
              and enc.hash_table.dtype == torch.float32 and getattr(enc, 'table_dtype', torch.float32) == torch.float32
              and lv.n_levels == LEVELS and lv.n_features == FEATURES and float(enc.base_res) == BASE_RES and enc.max_params == 2**LOG2_T
              and abs(enc.log_b - np.log(MAX_RES / BASE_RES) / (LEVELS - 1)) <= 1e-6 * enc.log_b
              and float(model.scale) == SCALE and model.cascades == CASCADES and model.grid_size == GRID_SIZE)
        if ok:
            xe, rn = model.xyz_encoder, model.rgb_net
            ok = (len(xe.hidden_layers) == 1 and len(rn.hidden_layers) == 1 and not xe.bias_enabled and not rn.bias_enabled
                  and tuple(xe.hidden_layers[0].weight.shape) == (16, 16) and tuple(xe.output_layer.weight.shape) == (16, 16)
                  and tuple(rn.hidden_layers[0].weight.shape) == (16, 32) and tuple(rn.output_layer.weight.shape) == (3, 16))
        if not ok:
            raise ValueError("from_module needs an NGP of the deployment architecture: NGP(**%r)" % (DEPLOYMENT_CONFIG,))
        c = lambda t: t.detach().float().cpu().reshape(-1)
        rgb_out = torch.cat([rn.output_layer.weight.detach().float().cpu(), torch.zeros(13, 16)], 0)       # save_deployment_model's padding
        return cls(c(enc.hash_table).numpy(), torch.cat([c(xe.hidden_layers[0].weight), c(xe.output_layer.weight)]).numpy(),
                   torch.cat([c(rn.hidden_layers[0].weight), rgb_out.reshape(-1)]).numpy(), model.density_bitfield.detach().cpu().numpy(),
                   poses=poses, per_level_scale=enc.log_b, device=enc.hash_table.device if enc.hash_table.is_cuda else None)

    def arrays(self):
        """The four arrays as host numpy (what two loaders of one model must agree on)."""
        return {"hash_table": self.hash_table, "sigma_weights": self.sigma_weights, "rgb_weights": self.rgb_weights,
                "density_bitfield": self.density_bitfield}

    # ------------------------------------------------------------------------------------------ device side
    def _tensors(self):
        if self._dev is None:
            if not torch.cuda.is_available():
                raise RuntimeError("rendering a deployment model needs the GPU: libngp_hip has no CPU path")
            dev = self.device or torch.device("cuda", torch.cuda.current_device())
            t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
            self._dev = (t(self.hash_table), t(self.sigma_weights), t(self.rgb_weights), t(self.density_bitfield))
            self.device = dev
        return self._dev

    def _coarse_table(self):
        """The coarse 8^3-block occupancy bits of the fused renderer's march, built once per model on first use."""
        if self._coarse is None:
            self._coarse = ops.coarse_bitfield(self._tensors()[3], CASCADES, GRID_SIZE)
        return self._coarse

    def shade(self, xyzs, dirs, return_enc=False):
        """World positions [n,3] in [-0.5, 0.5], directions [n,3] -> (sigmas [n], rgbs [n,3]) (+ the [n,16] embedding)."""
        table, sw, rw, _ = self._tensors()
        return ops.deploy_shade(xyzs.contiguous(), dirs.contiguous(), table, self.levels, sw, rw, return_enc=return_enc)

    @torch.no_grad()
    def render(self, pose, directions=None, res=(300, 600), camera_angle_x=0.5, T_threshold=1e-2, max_samples=None, mode="oneshot"):
        """pose: 3x4 camera-to-world.  directions: [N,3] camera-frame directions, default get_directions(*res, camera_angle_x) with
        res = (width, height).  The colour is accumulated over black, as the reference's run_inference leaves it.
        mode="oneshot": every ray is marched to the end of the box (at most max_samples occupied steps, default 1024), shaded and
        composited front to back until T <= T_threshold.  mode="progressive": the reference's rounds -- every alive ray advances by
        N_samples = max(min(N_rays // N_alive, 64), 1) occupied steps per round until the summed round budgets reach max_samples
        (default 100); rays still alive then keep what they have accumulated.  mode="fused": one-shot's image from ONE launch behind
        get_rays -- every ray is marched, shaded and composited by its own lane and its march ends where its composite does (at most
        max_samples composited samples, default 1024); no per-sample arrays, no chunk loop, no host read.
        -> {'rgb': [N,3], 'opacity': [N], 'depth': [N], 'total_samples': int64 tensor} on the device; progressive mode adds 'schedule'
        (the (N_alive, N_samples) of every round) and 'alive' (the rays the budget ran out on), fused mode 'n_samples' ([N] int32, the
        composited samples of every ray; one-shot counts the same samples in total_samples)."""
        if mode not in ("oneshot", "progressive", "fused"):
            raise ValueError("mode must be 'oneshot', 'progressive' or 'fused', got %r" % (mode,))
        _, _, _, bits = self._tensors()
        dev = self.device
        if directions is None:
            directions = get_directions(res[0], res[1], camera_angle_x)
        directions = torch.as_tensor(directions, dtype=torch.float32).reshape(-1, 3).to(dev).contiguous()
        if torch.is_tensor(pose):
            pose = pose.detach().to(dev, torch.float32).reshape(3, 4)      # a device pose stays there: no host read in front of the frame
        else:
            pose = torch.as_tensor(np.asarray(pose, np.float32).reshape(3, 4)).to(dev)
        from .rays import get_rays
        rays_o, rays_d = get_rays(directions, pose)            # rays_d = directions @ pose[:, :3].T (k = 0, 1, 2 in order), origin pose[:, 3]
        if mode == "fused":
            return self._render_fused(rays_o, rays_d, bits, T_threshold, 1024 if max_samples is None else int(max_samples))
        hits_t = ops.ray_aabb(rays_o, rays_d, SCALE)           # the slab test of modules/intersection.py, near plane 0.01
        if mode == "progressive":
            return self._render_progressive(rays_o, rays_d, hits_t, bits, T_threshold, 100 if max_samples is None else int(max_samples))
        return self._render_oneshot(rays_o, rays_d, hits_t, bits, T_threshold, 1024 if max_samples is None else int(max_samples))

    def _render_oneshot(self, rays_o, rays_d, hits_t, bits, T_threshold, max_samples):
        n, dev = rays_o.shape[0], rays_o.device
        opacity, depth, rgb = torch.zeros(n, device=dev), torch.zeros(n, device=dev), torch.zeros(n, 3, device=dev)
        total = torch.zeros((), device=dev, dtype=torch.int64)
        for a in range(0, n, RENDER_CHUNK):
            b = min(a + RENDER_CHUNK, n)
            noise = torch.zeros(b - a, device=dev)
            rays_a, xyzs, dirs, deltas, ts, _ = ops.march_train(rays_o[a:b], rays_d[a:b], hits_t[a:b].contiguous(), bits, noise, CASCADES, SCALE,
                                                                0.0, GRID_SIZE, max_samples)
            if xyzs.shape[0] == 0:
                continue
            sigmas, rgbs = self.shade(xyzs, dirs)
            vr, op_c, dep_c, rgb_c, _ = ops.composite_train_fwd(sigmas, rgbs, deltas, ts, rays_a, T_threshold)
            opacity[a:b] = op_c; depth[a:b] = dep_c; rgb[a:b] = rgb_c
            total += vr.sum()
        return {'rgb': rgb, 'opacity': opacity, 'depth': depth, 'total_samples': total}

    def _render_fused(self, rays_o, rays_d, bits, T_threshold, max_samples):
        table, sw, rw, _ = self._tensors()
        rgb, opacity, depth, n_samples, _ = ops.deploy_render(rays_o, rays_d, bits, self._coarse_table(), table, self.levels, sw, rw,
                                                              T_threshold, max_samples)
        return {'rgb': rgb, 'opacity': opacity, 'depth': depth, 'total_samples': n_samples.sum(dtype=torch.int64), 'n_samples': n_samples}

    def _render_progressive(self, rays_o, rays_d, hits_t, bits, T_threshold, max_samples):
        n, dev = rays_o.shape[0], rays_o.device
        opacity, depth, rgb = torch.zeros(n, device=dev), torch.zeros(n, device=dev), torch.zeros(n, 3, device=dev)
        alive = torch.arange(n, device=dev)
        marched = 0
        total = torch.zeros((), device=dev, dtype=torch.int64)
        rounds = []
        while marched < max_samples and len(alive) > 0:
            n_step = max(min(n // len(alive), 64), 1)
            marched += n_step
            rounds.append((len(alive), n_step))
            ray_indices, valid, deltas, ts, counter = ops.march_test(rays_o, rays_d, hits_t, alive, bits, CASCADES, SCALE, 0.0, GRID_SIZE, n_step)
            valid = valid.bool()
            counts = counter.to(torch.int64)
            pack_info = torch.stack([torch.cumsum(counts, 0) - counts, counts], -1).contiguous()
            ray_indices, deltas, ts = ray_indices[valid], deltas[valid].contiguous(), ts[valid].contiguous()
            if ray_indices.shape[0] > 0:
                d = rays_d[ray_indices]
                sigmas, rgbs = self.shade(rays_o[ray_indices] + ts[:, None] * d, d)
            else:
                sigmas, rgbs = torch.zeros(0, device=dev), torch.zeros(0, 3, device=dev)
            ops.composite_test(sigmas, rgbs, deltas, ts, pack_info, alive, T_threshold, opacity, depth, rgb)   # marks finished rays -1
            alive = alive[alive >= 0]
            total += counts.sum()
        return {'rgb': rgb, 'opacity': opacity, 'depth': depth, 'total_samples': total, 'schedule': rounds, 'alive': alive}
