"""numpy restatement of the deployment model's inference (csrc/deploy.hip, ngp_hip/deploy.py), used by tests/test_deploy.py and
tests/test_gpu_deploy.py: the level table, the dense-grid embedding with the training encoder's modulo rule, the 16 SH terms, the two
16-wide networks and the camera directions.  dtype=np.float32 evaluates every operation as a separate binary32 multiply or add in the
order of the reference's loops (numpy never contracts); dtype=np.float64 is the same graph in double, the yardstick the tolerances of
profiles/PARITY_NOTES.md are measured against."""
import numpy as np

BASE_RES, MAX_RES, LEVELS, FEATURES, LOG2_T = 32, 128, 4, 4, 21
LOG_B = float(np.log(MAX_RES / BASE_RES) / (LEVELS - 1))
TOTAL_ENTRIES = 2794024
BITFIELD_BYTES = 128**3 // 8

# (sigma relative, rgb absolute) bounds of the per-sample rows of tests/golden/ref_deploy.npz, per weight set: 4x the distance of the
# reference's own f32 result from the float64 restatement (lego: 7.886e-5 / 4.293e-6, syn: 9.562e-6 / 4.631e-6), rounded up to two
# digits.  tests/test_deploy.py re-measures them; profiles/PARITY_NOTES.md has the derivation.
BOUNDS = {"lego": (3.2e-4, 1.8e-5), "syn": (3.9e-5, 1.9e-5)}


def level_table(log_b=LOG_B):
    """(scale f32[4], resolution, map_size, offset) of the 4-level table: hash_encoder.py:183-205 with max_params 2^21."""
    scale = np.float32(BASE_RES) * np.exp(np.arange(LEVELS, dtype=np.float32) * np.float32(log_b)) - np.float32(1.0)
    res = (np.ceil(scale).astype(np.uint32) + 1).astype(np.uint32)
    size, offset, off = [], [], 0
    for l in range(LEVELS):
        full = int(np.ceil(BASE_RES * np.exp(l * float(log_b)) - 1.0) + 1)**3
        s = min(2**LOG2_T, (full + 7) // 8 * 8)
        offset.append(off); size.append(s)
        off += s
    return scale.astype(np.float32), res, np.array(size, np.uint32), np.array(offset, np.uint32)


def synthetic_table(amplitude, n=TOTAL_ENTRIES * FEATURES):
    """The seeded table of the fixtures (oracle.gen_golden.golden_table's closed form spread over [-amplitude, amplitude))."""
    i = np.arange(n, dtype=np.uint64)
    h = (i * np.uint64(2654435761) + np.uint64(12345)) % np.uint64(2**32)
    return (-amplitude + 2.0 * amplitude * (h.astype(np.float64) / 2**32)).astype(np.float32)


def corner_indices(xyz, levels):
    """Unwrapped dense corner indices x + y res + z res^2, [n, 4, 8] int64, and the level sizes: the reference's deployment kernel
    (which applies no modulo) stays inside a level exactly where index < size."""
    scale, res, size, _ = levels
    x01 = np.asarray(xyz, np.float32) + np.float32(0.5)
    out = np.empty((x01.shape[0], LEVELS, 8), np.int64)
    for l in range(LEVELS):
        pos = x01 * scale[l] + np.float32(0.5)
        cell = np.floor(pos).astype(np.int64)
        for ci in range(8):
            g = [cell[:, d] + ((ci >> d) & 1) for d in range(3)]
            out[:, l, ci] = g[0] + g[1] * int(res[l]) + g[2] * int(res[l])**2
    return out, size.astype(np.int64)


def embed(xyz, table, levels, dtype=np.float32):
    """[n,3] world positions -> [n,16]: x01 = xyz + 0.5, trilinear gather of 4 features on 4 dense levels, index % map_size."""
    scale, res, size, offset = levels
    T = np.asarray(table, np.float32).reshape(-1, FEATURES).astype(dtype)
    x01 = np.asarray(xyz, np.float32).astype(dtype) + dtype(0.5)
    out = np.zeros((x01.shape[0], LEVELS * FEATURES), dtype)
    for l in range(LEVELS):
        pos = x01 * dtype(scale[l]) + dtype(0.5)
        cellf = np.floor(pos)
        cell = np.clip(cellf, 0, 4294967295.0).astype(np.uint64)                 # the kernel's saturating f32 -> u32 cast
        fr = pos - cell.astype(dtype)
        acc = np.zeros((x01.shape[0], FEATURES), dtype)
        for ci in range(8):
            w = np.ones(x01.shape[0], dtype)
            g = []
            for d in range(3):
                if (ci >> d) & 1:
                    g.append((cell[:, d] + 1) & 0xffffffff); w = w * fr[:, d]
                else:
                    g.append(cell[:, d]); w = w * (dtype(1.0) - fr[:, d])
            h = (g[0] + g[1] * int(res[l]) + g[2] * (int(res[l])**2 & 0xffffffff)) & 0xffffffff        # u32 arithmetic
            idx = (h % int(size[l])).astype(np.int64) + int(offset[l])
            acc = acc + w[:, None] * T[idx]
        out[:, 4 * l:4 * l + 4] = acc
    return out


def sh16(dirs, dtype=np.float32):
    d = np.asarray(dirs, np.float32).astype(dtype)
    nrm = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
    d = (d / nrm[:, None] + dtype(1.0)) / dtype(2.0)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    xy, xz, yz, x2, y2, z2 = x * y, x * z, y * z, x * x, y * y, z * z
    c = dtype
    out = np.empty((d.shape[0], 16), dtype)
    out[:, 0] = c(0.28209479177387814)
    out[:, 1] = c(-0.48860251190291987) * y
    out[:, 2] = c(0.48860251190291987) * z
    out[:, 3] = c(-0.48860251190291987) * x
    out[:, 4] = c(1.0925484305920792) * xy
    out[:, 5] = c(-1.0925484305920792) * yz
    out[:, 6] = c(0.94617469575755997) * z2 - c(0.31539156525251999)
    out[:, 7] = c(-1.0925484305920792) * xz
    out[:, 8] = c(0.54627421529603959) * x2 - c(0.54627421529603959) * y2
    out[:, 9] = c(0.59004358992664352) * y * (c(-3.0) * x2 + y2)
    out[:, 10] = c(2.8906114426405538) * xy * z
    out[:, 11] = c(0.45704579946446572) * y * (c(1.0) - c(5.0) * z2)
    out[:, 12] = c(0.3731763325901154) * z * (c(5.0) * z2 - c(3.0))
    out[:, 13] = c(0.45704579946446572) * x * (c(1.0) - c(5.0) * z2)
    out[:, 14] = c(1.4453057213202769) * z * (x2 - y2)
    out[:, 15] = c(0.59004358992664352) * x * (-x2 + c(3.0) * y2)
    return out


def _seq_matvec(x, W, dtype):
    """x [n, k] times W [o, k]^T with every output summed over k in index order from 0."""
    out = np.zeros((x.shape[0], W.shape[0]), dtype)
    for j in range(W.shape[1]):
        out = out + x[:, j:j + 1] * W[None, :, j]
    return out


def mlp(enc, dirs, sigma_w, rgb_w, dtype=np.float32):
    """enc [n,16], raw directions -> (log sigma [n], sigma [n], rgb [n,3]) with save_deployment_model's weight layout."""
    sw, rw = np.asarray(sigma_w, np.float32).astype(dtype), np.asarray(rgb_w, np.float32).astype(dtype)
    W1, W2 = sw[:256].reshape(16, 16), sw[256:512].reshape(16, 16)
    W3, W4 = rw[:512].reshape(16, 32), rw[512:768].reshape(16, 16)[:3]
    h = _seq_matvec(np.maximum(_seq_matvec(np.asarray(enc).astype(dtype), W1, dtype), dtype(0.0)), W2, dtype)
    x = np.concatenate([sh16(dirs, dtype), h], 1)
    s = _seq_matvec(np.maximum(_seq_matvec(x, W3, dtype), dtype(0.0)), W4, dtype)
    return h[:, 0], np.exp(h[:, 0]), dtype(1.0) / (dtype(1.0) + np.exp(-s))


def shade(xyz, dirs, table, levels, sigma_w, rgb_w, dtype=np.float32):
    enc = embed(xyz, table, levels, dtype)
    _, sigma, rgb = mlp(enc, dirs, sigma_w, rgb_w, dtype)
    return enc, sigma, rgb


def directions(res_w, res_h, camera_angle_x=0.5):
    """Camera-frame directions of a res_w x res_h image, [h*w, 3] f32, row-major over (row, column): pixel centres, one focal length
    per axis from the same angle (kernels.py:595-607)."""
    w, h = int(res_w), int(res_h)
    fx, fy = 0.5 * w / np.tan(0.5 * camera_angle_x), 0.5 * h / np.tan(0.5 * camera_angle_x)
    x, y = np.meshgrid(np.arange(w, dtype=np.float32) + 0.5, np.arange(h, dtype=np.float32) + 0.5, indexing='xy')
    return np.stack([(x - 0.5 * w) / fx, (y - 0.5 * h) / fy, np.ones_like(x)], -1).reshape(-1, 3).astype(np.float32)


def render_progressive(ora, pose, dirs_cam, bitfield, table, levels, sigma_w, rgb_w, T_threshold=1e-2, max_samples=100):
    """The reference's run_inference loop on the CPU oracle's march / composite with the restated shading between them.
    -> (rgb [N,3], opacity [N], depth [N], schedule [(N_alive, N_samples)], total samples, per-ray end state: 0 no samples left in the box,
    1 ended by T_threshold, 2 still alive when the round budget ran out)."""
    rays_o, rays_d = ora.get_rays(dirs_cam, np.asarray(pose, np.float32).reshape(3, 4))
    n = rays_o.shape[0]
    hits = np.ascontiguousarray(ora.ray_aabb(rays_o, rays_d, 0.5))
    opacity, depth, rgb = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros((n, 3), np.float32)
    alive = np.arange(n, dtype=np.int64)
    state = np.zeros(n, np.int32)
    marched, total, schedule = 0, 0, []
    while marched < max_samples and len(alive):
        n_step = max(min(n // len(alive), 64), 1)
        marched += n_step
        schedule.append((len(alive), n_step))
        ri, valid, deltas, ts, counter = ora.march_test(rays_o, rays_d, hits, alive, bitfield, 1, 0.5, 0.0, 128, n_step)
        m = valid.astype(bool)
        ri, deltas, ts = ri[m], deltas[m], ts[m]
        counts = counter.astype(np.int64)
        pack = np.stack([np.cumsum(counts) - counts, counts], -1)
        total += int(counts.sum())
        xyz = rays_o[ri] + ts[:, None] * rays_d[ri]
        _, sigma, rgbs = shade(xyz, rays_d[ri], table, levels, sigma_w, rgb_w)
        before = alive.copy()
        ora.composite_test(sigma, rgbs, deltas, ts, pack, alive, T_threshold, opacity, depth, rgb)
        ended = alive < 0
        state[before[ended & (counts > 0)]] = 1
        state[before[ended & (counts == 0)]] = 0
        alive = alive[alive >= 0]
    state[alive] = 2
    return rgb, opacity, depth, schedule, total, state
