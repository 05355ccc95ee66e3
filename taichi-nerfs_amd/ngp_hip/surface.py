"""Surface rendering: a signed-distance field trained from images through the NeuS-opacity compositor (csrc/surface.hip).

`SurfaceRenderer` / `surface_render_func`  the autograd node over ngp_surface_composite_fwd / _bwd
`SDFField`                                 hash encoder (twice differentiable) + a small geometry MLP -> (sdf, feature), a colour MLP on
                                           (feature, normal, SH16(dir)), one learnable sharpness, and the occupancy grid the march reads
`trace_surface`, `render_surface_traced`   test-time rendering by sphere tracing (csrc/sdf_trace.hip): one launch walks every ray to the zero
                                           crossing, then sdf_and_grad and color run on that one point per ray
`render_surface`                           slab test -> march -> (n_importance > 0: a coarse pass and ops.resample_rays, csrc/resample.hip)
                                           -> sdf and its gradient -> colours -> compositor -> result dictionary

The opacity of a sample comes from the signed distance f, the directional derivative dir . grad f and the global inverse standard
deviation s = exp(log_inv_s) (contract: include/ngp_hip.h).  grad f is taken by autograd through the hash encoder's position gradient;
with create_graph=True a loss on it (the eikonal term, the normals the colour MLP sees) trains the table through the encoder's double
backward.  The MLPs are plain torch layers."""
import math

import torch
from torch import nn

from . import ops as _ops

MAX_SAMPLES = 1024


class SurfaceRenderer(torch.autograd.Function):
    """(sdf [S], cosv [S], rgbs [S,3], aux [S,3] | None, deltas, ts, rays_a [n,3] i32, inv_s [1 element, device], cos_anneal, T_threshold,
    bg) -> (vr_samples, opacity [n], depth [n], rgb [n,3] blended over bg, ws [S], aux_out [n,3] | None, alphas [S]).  Differentiable
    with respect to sdf, cosv, rgbs, aux and inv_s; deltas and ts get no gradient, as in VolumeRenderer."""

    @staticmethod
    def forward(ctx, sdf, cosv, rgbs, aux, deltas, ts, rays_a, inv_s, cos_anneal, T_threshold, bg):
        total, opacity, depth, _rgb, rgb_out, aux_out, ws, alphas = _ops.surface_composite_fwd(
            sdf, cosv, rgbs, deltas, ts, rays_a, inv_s, cos_anneal, T_threshold, aux, bg)
        ctx.cos_anneal, ctx.bg, ctx.has_aux = float(cos_anneal), float(bg), aux is not None
        ctx.save_for_backward(sdf, cosv, rgbs, aux, deltas, ts, rays_a, inv_s, total, alphas)
        ctx.set_materialize_grads(False)
        vr = total.sum()
        ctx.mark_non_differentiable(vr, alphas)
        return vr, opacity, depth, rgb_out, ws, aux_out, alphas

    @staticmethod
    def backward(ctx, _g_vr, g_opacity, g_depth, g_rgb, g_ws, g_aux, _g_alphas):
        sdf, cosv, rgbs, aux, deltas, ts, rays_a, inv_s, total, alphas = ctx.saved_tensors

        def f32(g):
            return None if g is None else g.contiguous().float()

        g_rgb = f32(g_rgb)
        if g_rgb is None:
            g_rgb = torch.zeros(rays_a.shape[0], 3, device=sdf.device, dtype=torch.float32)
        d_sdf, d_cos, d_rgbs, d_aux, d_inv_s = _ops.surface_composite_bwd(
            f32(g_opacity), f32(g_depth), g_rgb, f32(g_aux) if ctx.has_aux else None, f32(g_ws), sdf, cosv, rgbs, deltas, ts, rays_a, inv_s,
            total, alphas, ctx.cos_anneal, aux, ctx.bg)
        return d_sdf, d_cos, d_rgbs, d_aux, None, None, None, d_inv_s.view(inv_s.shape), None, None, None


def surface_render_func(sdf, cosv, rgbs, deltas, ts, rays_a, inv_s, cos_anneal=1.0, T_threshold=1e-4, aux=None, bg=0.0):
    """-> (vr_samples, opacity, depth, rgb, ws, aux_out); rgb is blended over bg, aux_out is None without aux."""
    c = lambda t: t.contiguous().float()
    return SurfaceRenderer.apply(c(sdf), c(cosv), c(rgbs), None if aux is None else c(aux), c(deltas), c(ts), rays_a.contiguous(),
                                 inv_s.contiguous().float(), cos_anneal, T_threshold, bg)[:6]


def _geometric_init(layers, radius):
    """The sphere initialisation of implicit-surface MLPs (Atzmon & Lipman, SAL; Gropp et al., IGR): hidden weights N(0, 2 / out), the
    last layer ~ sqrt(pi / width) with bias -radius.  With a sharp Softplus the fresh network is close to |x| - radius as long as its
    input is little more than the three coordinates -- the encoding's share is kept out not by zeroing its first-layer columns (the
    table would then start without a gradient) but by starting the table at +-1e-4."""
    with torch.no_grad():
        for i, lin in enumerate(layers):
            out = lin.out_features
            if i == len(layers) - 1:
                nn.init.normal_(lin.weight, mean=math.sqrt(math.pi) / math.sqrt(lin.in_features), std=1e-4)
                nn.init.constant_(lin.bias, -radius)
                lin.weight[1:].normal_(0.0, 1e-4)                  # the feature rows: small, they are not a distance
                lin.bias[1:].zero_()
            else:
                nn.init.normal_(lin.weight, 0.0, math.sqrt(2.0) / math.sqrt(out))
                nn.init.constant_(lin.bias, 0.0)


class SDFField(nn.Module):
    """A signed-distance field with view-dependent colour on the unit-scale box [-scale, scale]^3.

    sdf(x), sdf_and_grad(x, create_graph), color(feature, normal, dirs), density(x) = s sigmoid(-s sdf(x)) -- the direction-free upper
    bound of NeuS's opaque density, what the occupancy update thresholds --, update_density_grid / mark_invisible_cells as on NGP."""

    def __init__(self, scale: float = 0.5, levels: int = 16, feature_per_level: int = 2, log2_T: int = 19, base_res: int = 16,
                 max_res: int = 2048, geo_width: int = 64, geo_depth: int = 2, feature_dim: int = 15, rgb_width: int = 64,
                 init_radius: float = 0.25, init_inv_s: float = 20.0):
        super().__init__()
        from modules.hash_encoder import HashEncoder
        from modules.networks import _cell_coords
        from modules.spherical_harmonics import DirEncoder
        self.scale = scale
        self.register_buffer('xyz_min', -torch.ones(1, 3) * scale)
        self.register_buffer('xyz_max', torch.ones(1, 3) * scale)
        self.cascades = max(1 + int(math.ceil(math.log2(2 * scale))), 1)
        self.grid_size = 128
        G3 = self.grid_size**3
        self.register_buffer('density_bitfield', torch.zeros(self.cascades * G3 // 8, dtype=torch.uint8))
        self.register_buffer('density_grid', torch.zeros(self.cascades, G3))
        self.register_buffer('grid_coords', _cell_coords(self.grid_size))

        self.pos_encoder = HashEncoder(max_params=2**log2_T, base_res=base_res, max_res=max_res, levels=levels,
                                       feature_per_level=feature_per_level, twice_differentiable=True)
        with torch.no_grad():                                      # features around 0: the fresh field is the MLP's sphere
            self.pos_encoder.hash_table.uniform_(-1e-4, 1e-4)
        dims = [3 + self.pos_encoder.out_dim] + [geo_width] * geo_depth + [1 + feature_dim]
        self.geo_layers = nn.ModuleList(nn.Linear(a, b) for a, b in zip(dims[:-1], dims[1:]))
        _geometric_init(self.geo_layers, init_radius)
        self.act = nn.Softplus(beta=100.0)
        self.dir_encoder = DirEncoder()
        self.rgb_net = nn.Sequential(nn.Linear(feature_dim + 3 + self.dir_encoder.out_dim, rgb_width), nn.ReLU(),
                                     nn.Linear(rgb_width, rgb_width), nn.ReLU(), nn.Linear(rgb_width, 3), nn.Sigmoid())
        self.log_inv_s = nn.Parameter(torch.tensor([math.log(init_inv_s)]))

    # ------------------------------------------------------------------------------------------ geometry
    def inv_s(self):
        return torch.exp(self.log_inv_s)

    def _geometry(self, x):
        x01 = (x - self.xyz_min) / (self.xyz_max - self.xyz_min)
        h = torch.cat([x, self.pos_encoder(x01).float()], 1)
        for lin in self.geo_layers[:-1]:
            h = self.act(lin(h))
        out = self.geo_layers[-1](h)
        return out[:, 0], out[:, 1:]

    def sdf(self, x):
        """x: [N,3] in [-scale, scale] -> signed distance [N] (negative inside)."""
        return self._geometry(x.contiguous().float())[0]

    def sdf_and_grad(self, x, create_graph=False):
        """-> (sdf [N], feature [N,F], grad [N,3] = d sdf / d x).  Runs under torch.enable_grad() on a detached copy of x (on x itself
        where it requires grad), so it works inside torch.no_grad().  create_graph=False: the three results are detached.
        create_graph=True: they carry the graph, and a loss on grad trains the table through the encoder's double backward."""
        with torch.enable_grad():
            xg = x if (create_graph and x.requires_grad) else x.detach().clone().requires_grad_(True)
            f, feat = self._geometry(xg)
            (grad,) = torch.autograd.grad(f.sum(), xg, create_graph=create_graph)
        if not create_graph:
            return f.detach(), feat.detach(), grad.detach()
        return f, feat, grad

    def color(self, feature, normal, dirs):
        """dirs: unit vectors.  -> rgb [N,3] in (0, 1)."""
        sh = self.dir_encoder(((dirs + 1) / 2).contiguous()).float()
        return self.rgb_net(torch.cat([feature, normal, sh], 1))

    def packed_geometry(self):
        """A fresh fp32 pack of the geometry MLP for the sphere tracer (ops.sdf_pack: W0 | b0 | .. | w_out | b_out, of the last layer
        row 0 alone) from the CURRENT parameters -- a copy: later training steps do not reach it."""
        return _ops.sdf_pack(self.geo_layers)

    def _trace_arch(self):
        return self.geo_layers[0].out_features, len(self.geo_layers) - 1

    @torch.no_grad()
    def sdf_fused(self, x, wpack=None):
        """sdf(x) through the tracer's field kernel (ops.sdf_eval): one launch, no graph."""
        width, depth = self._trace_arch()
        enc = self.pos_encoder
        return _ops.sdf_eval(x.contiguous().float(), enc.hash_table.detach().contiguous(), enc._levels,
                             self.packed_geometry() if wpack is None else wpack, width, depth, self.scale)

    def density(self, x):
        s = self.inv_s().detach()
        return s * torch.sigmoid(-s * self.sdf(x))

    # ------------------------------------------------------------------------------------------ occupancy grid (NGP's algorithm)
    def get_all_cells(self):
        from modules.networks import NGP
        return NGP.get_all_cells(self)

    def sample_uniform_and_occupied_cells(self, M, density_threshold):
        from modules.networks import NGP
        return NGP.sample_uniform_and_occupied_cells(self, M, density_threshold)

    def mark_invisible_cells(self, K, poses, img_wh, chunk=32**3):
        from modules.networks import NGP
        return NGP.mark_invisible_cells(self, K, poses, img_wh, chunk)

    @torch.no_grad()
    def update_density_grid(self, density_threshold, warmup=False, decay=0.95, erode=False, jitter=None):
        from modules.networks import _merge_fresh_densities
        from modules.utils import packbits
        if jitter is not None and not warmup:
            raise ValueError("an explicit jitter is defined for the warm-up form (all cells) only")
        _merge_fresh_densities(self, density_threshold, warmup, decay, erode, jitter)
        mean_density = self.density_grid[self.density_grid > 0].mean().item()
        packbits(self.density_grid.reshape(-1).contiguous(), min(mean_density, density_threshold), self.density_bitfield)


def _refine(model, rays_o, rays_d, noise, rays_a, xyzs, dirs, deltas, ts, n_importance, importance_inv_s, cos_anneal, T_threshold):
    """The coarse pass of hierarchical sampling: f and dir . grad f on the marched samples (no graph; grad mode is on for grad f alone),
    the compositor's ws at importance_inv_s (None: the model's own sharpness), then n_importance inverse-CDF draws per ray with the
    ray's march jitter.  The refined positions are detached, as in NeRF and NeuS."""
    with torch.no_grad():
        f, _, g = model.sdf_and_grad(xyzs, create_graph=False)
        cosv = (dirs * g).sum(1)
        if importance_inv_s is None:
            inv_s = model.inv_s().detach()
        else:
            inv_s = torch.full((1,), float(importance_inv_s), device=xyzs.device)
        ws = _ops.surface_composite_fwd(f.contiguous(), cosv.contiguous(), torch.zeros_like(xyzs), deltas, ts, rays_a, inv_s.contiguous(),
                                        cos_anneal, T_threshold)[6]
        return _ops.resample_rays(ws, deltas, ts, rays_a, rays_o, rays_d, noise, n_importance)


def _render_chunk(model, rays_o, rays_d, noise, grad, cos_anneal, T_threshold, max_samples, bg, n_importance=0, importance_inv_s=None):
    hits_t = _ops.ray_aabb(rays_o, rays_d, model.scale)
    rays_a, xyzs, dirs, deltas, ts, total = _ops.march_train(rays_o, rays_d, hits_t, model.density_bitfield, noise, model.cascades,
                                                             model.scale, 0.0, model.grid_size, max_samples)
    extra = {}
    if n_importance > 0:
        extra['rm_samples_coarse'] = total
        if xyzs.shape[0]:
            rays_a, xyzs, dirs, deltas, ts, parent, total = _refine(model, rays_o, rays_d, noise, rays_a, xyzs, dirs, deltas, ts,
                                                                    n_importance, importance_inv_s, cos_anneal, T_threshold)
        else:
            parent = torch.zeros(0, device=rays_o.device, dtype=torch.int32)
        extra['parent'] = parent
    if xyzs.shape[0] == 0:                                     # nothing marched: every ray shows the background
        z = torch.zeros(0, device=rays_o.device)
        f, feat, g = z, torch.zeros(0, model.geo_layers[-1].out_features - 1, device=rays_o.device), torch.zeros(0, 3, device=rays_o.device)
    else:
        f, feat, g = model.sdf_and_grad(xyzs, create_graph=grad)
    grad_norm = torch.linalg.norm(g, dim=1)
    normal = g / grad_norm.clamp_min(1e-12)[:, None]
    cosv = (dirs * g).sum(1)
    rgbs = model.color(feat, normal, dirs) if xyzs.shape[0] else torch.zeros(0, 3, device=rays_o.device)
    inv_s = model.inv_s() if grad else model.inv_s().detach()
    if grad:
        vr, opacity, depth, rgb, ws, aux_out, alphas = SurfaceRenderer.apply(
            f.contiguous(), cosv.contiguous(), rgbs.contiguous().float(), normal.contiguous(), deltas, ts, rays_a, inv_s.contiguous(),
            cos_anneal, T_threshold, bg)
    else:
        tot, opacity, depth, _rgb, rgb, aux_out, ws, alphas = _ops.surface_composite_fwd(
            f.contiguous(), cosv.contiguous(), rgbs.contiguous().float(), deltas, ts, rays_a, inv_s.contiguous(), cos_anneal,
            T_threshold, normal.contiguous(), bg)
        vr = tot.sum()
    return dict({'rgb': rgb, 'opacity': opacity, 'depth': depth, 'normal': aux_out, 'ws': ws, 'alphas': alphas, 'rays_a': rays_a,
                 'grad_norm': grad_norm, 'deltas': deltas, 'ts': ts, 'rm_samples': total, 'vr_samples': vr}, **extra)


def render_surface(model, rays_o, rays_d, test_time=False, cos_anneal=1.0, T_threshold=1e-4, max_samples=MAX_SAMPLES, bg=1.0,
                   chunk=16384, n_importance=0, importance_inv_s=None):
    """rays_o, rays_d: [N,3] (directions are normalised here: t, depth and the SDF share one unit).  -> dict rgb [N,3] (blended over
    bg), opacity, depth [N], normal [N,3] (the composited unit normals), ws, alphas, grad_norm [S] (|grad f| per sample, for the eikonal
    term), rays_a, deltas, ts, rm_samples, vr_samples.

    n_importance > 0: hierarchical sampling.  A first pass without a graph takes the compositor's weights on the marched samples at
    importance_inv_s (None: the model's own sharpness) and cuts the marched sections with n_importance inverse-CDF draws per ray
    (ops.resample_rays, the ray's march jitter as the draw's); everything above is then rendered on the refined samples.  The dict
    gains parent [S] i32 (the marched sample each refined one was cut from) and rm_samples_coarse (the march's count).  With
    n_importance = 0 nothing of this is launched.

    Training (test_time=False): jittered march, everything differentiable (the model must be in grad mode).  test_time=True: zero
    jitter, `chunk` rays at a time, no graph -- usable inside torch.no_grad(); grad mode is switched on internally for grad f only.
    Per-sample entries of a chunked render are those of the LAST chunk; the per-ray ones cover every ray."""
    rays_o = rays_o.contiguous().float()
    rays_d = rays_d.float()
    rays_d = (rays_d / torch.linalg.norm(rays_d, dim=1, keepdim=True)).contiguous()
    n = rays_o.shape[0]
    if not test_time:
        noise = torch.rand(n, device=rays_o.device)
        return _render_chunk(model, rays_o, rays_d, noise, True, cos_anneal, T_threshold, max_samples, bg, n_importance, importance_inv_s)
    out = None
    per_ray = {k: [] for k in ('rgb', 'opacity', 'depth', 'normal')}
    rm, vr, rm_coarse = 0, 0, 0
    with torch.no_grad():
        for a in range(0, n, chunk):
            b = min(a + chunk, n)
            out = _render_chunk(model, rays_o[a:b].contiguous(), rays_d[a:b].contiguous(), torch.zeros(b - a, device=rays_o.device), False,
                                cos_anneal, T_threshold, max_samples, bg, n_importance, importance_inv_s)
            for k in per_ray:
                per_ray[k].append(out[k])
            rm, vr = rm + out['rm_samples'], vr + out['vr_samples']
            rm_coarse = rm_coarse + out.get('rm_samples_coarse', 0)
    if out is None:
        raise ValueError("render_surface needs at least one ray")
    out.update({k: torch.cat(v) for k, v in per_ray.items()}, rm_samples=rm, vr_samples=vr)
    if n_importance > 0:
        out['rm_samples_coarse'] = rm_coarse
    return out


@torch.no_grad()
def trace_surface(model, rays_o, rays_d, wpack=None, coarse=None, out=None, stats=None, **params):
    """Sphere tracing of an SDFField (ops.sdf_trace; the rule is the "sphere tracing" block of include/ngp_hip.h): rays_o [N,3], rays_d
    [N,3] UNIT vectors -> dict status [N] i32 (0 MISS, 1 HIT, 2 INSIDE, 3 ABANDONED), t [N], xyz [N,3], n_eval [N] i32, f_last [N].
    params: eps, step_scale, min_step, n_refine, max_evals.  wpack / coarse: model.packed_geometry() / the coarse occupancy bits, to
    reuse them over several calls; by default both are made here."""
    width, depth = model._trace_arch()
    enc = model.pos_encoder
    if wpack is None:
        wpack = model.packed_geometry()
    if coarse is None:
        coarse = _ops.coarse_bitfield(model.density_bitfield, model.cascades, model.grid_size)
    res = _ops.sdf_trace(rays_o, rays_d, model.density_bitfield, coarse, enc.hash_table.detach().contiguous(), enc._levels, wpack, width,
                         depth, model.cascades, model.scale, model.grid_size, out=out, stats=stats, **params)
    return dict(zip(("status", "t", "xyz", "n_eval", "f_last"), res))


def render_surface_traced(model, rays_o, rays_d, bg=1.0, chunk=1 << 20, **params):
    """Test-time rendering by sphere tracing: rays_o, rays_d [N,3] (directions are normalised here) -> dict rgb [N,3], opacity, depth [N],
    normal [N,3], status, n_eval [N] i32.  The trace runs `chunk` rays per launch; sdf_and_grad and color then run on the HIT and
    INSIDE points only, one per ray: rgb = the shaded colour, opacity 1, depth t, normal grad f / |grad f|.  Every other ray shows
    bg with opacity, depth and normal 0.  No graph is kept: usable inside torch.no_grad() (grad mode is switched on for grad f alone)."""
    rays_o = rays_o.contiguous().float()
    rays_d = rays_d.float()
    rays_d = (rays_d / torch.linalg.norm(rays_d, dim=1, keepdim=True)).contiguous()
    n, dev = rays_o.shape[0], rays_o.device
    if n == 0:
        raise ValueError("render_surface_traced needs at least one ray")
    with torch.no_grad():
        wpack = model.packed_geometry()
        coarse = _ops.coarse_bitfield(model.density_bitfield, model.cascades, model.grid_size)
        parts = [trace_surface(model, rays_o[a:a + chunk].contiguous(), rays_d[a:a + chunk].contiguous(), wpack=wpack, coarse=coarse, **params)
                 for a in range(0, n, chunk)]
        tr = {k: torch.cat([p[k] for p in parts]) for k in parts[0]}
        on = (tr["status"] == 1) | (tr["status"] == 2)
        rgb = torch.full((n, 3), float(bg), device=dev)
        normal = torch.zeros(n, 3, device=dev)
        idx = on.nonzero().squeeze(1)
        if idx.numel():
            _, feat, g = model.sdf_and_grad(tr["xyz"][idx].contiguous(), create_graph=False)
            nrm = g / torch.linalg.norm(g, dim=1).clamp_min(1e-12)[:, None]
            rgb[idx] = model.color(feat, nrm, rays_d[idx]).float()
            normal[idx] = nrm
        return {"rgb": rgb, "opacity": on.float(), "depth": torch.where(on, tr["t"], torch.zeros_like(tr["t"])), "normal": normal,
                "status": tr["status"], "n_eval": tr["n_eval"]}
