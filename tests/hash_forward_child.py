"""Child process of tests/test_gpu_hash_forward_exact.py (a plain script; pytest does not collect it).

NGP_EXPERIMENT is read once per process, so the loop variants of the forward hash gather it selects (hash_fwd_tiles, hash_fwd_v1) need
a process of their own.  This script reads an .npz of inputs, runs the forms it is told to over every size and both layouts into
buffers pre-filled with FILL (SPARE spare rows behind them), and writes an .npz of the raw buffers; the parent compares.

    python hash_forward_child.py IN.npz OUT.npz f32,bf16,f16,list_f32,list_bf16

IN.npz: shape (the five level-table numbers), x [n_max, 3], x_list [n_max, 3] (un-normalised positions of the list forms), lo_hi,
perm [n_max] int32 (the list of length n is perm[:n]), sizes, table_f32, table_bf16 (uint16 bit patterns), table_f16."""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "taichi-nerfs_amd"))

FILL, SPARE = -7.0, 64


def main(path_in, path_out, forms):
    import torch
    from ngp_hip import ops
    d = np.load(path_in)
    L = ops._lib()
    lv = ops.make_levels(*[int(v) for v in d["shape"]])
    dev = "cuda"
    x, x_list = torch.from_numpy(d["x"]).to(dev), torch.from_numpy(d["x_list"]).to(dev)
    lo, hi = float(d["lo_hi"][0]), float(d["lo_hi"][1])
    perm = torch.from_numpy(d["perm"]).to(dev)
    tables = {"f32": torch.from_numpy(d["table_f32"]).to(dev),
              "bf16": torch.from_numpy(d["table_bf16"].view(np.int16)).to(dev).view(torch.bfloat16),
              "f16": torch.from_numpy(d["table_f16"]).to(dev)}
    null = ctypes.c_void_p(0)
    res = {}
    for form in forms:
        for pairs in (0, 1):
            for n in [int(v) for v in d["sizes"]]:
                if form.startswith("list_"):        # the list form's buffer has n_max rows whatever the list's length
                    kind, n_max = form[5:], x.shape[0]
                    out = torch.full(((n_max + SPARE) * 32,), FILL, device=dev)
                    cnt = torch.tensor([n], device=dev, dtype=torch.int32)
                    rc = L.ngp_hash_fwd_list(ops._ptr(x_list), ops._ptr(tables[kind]), int(kind == "bf16"), ctypes.byref(lv), n_max,
                                             ops._ptr(cnt), ops._ptr(perm), 1, lo, hi, pairs, ops._ptr(out), ops._stream())
                else:
                    out = torch.full(((n + SPARE) * 32,), FILL, device=dev)
                    fn = {"f32": L.ngp_hash_fwd_f32_ex, "bf16": L.ngp_hash_fwd_bf16_ex, "f16": L.ngp_hash_fwd_f16_ex}[form]
                    rc = fn(ops._ptr(x), ops._ptr(tables[form]), ctypes.byref(lv), n, null, 0, 0.0, 1.0, pairs, ops._ptr(out), ops._stream())
                torch.cuda.synchronize()
                if rc != 0:
                    print("%s pairs=%d n=%d returned %d" % (form, pairs, n, rc))
                    return 3
                res["%s_%d_%d" % (form, pairs, n)] = out.cpu().numpy()
    np.savez(path_out, **res)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2], sys.argv[3].split(",")))
