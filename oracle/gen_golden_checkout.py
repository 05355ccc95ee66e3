"""Fixtures for the tests that used to read the reference checkout directly, so that they run where it is absent.  Run where the
checkout exists (the checkout oracle/gen_golden.py reads):

    python oracle/gen_golden_checkout.py

Writes
  * tests/golden/ref_kat_shim.npz: the reference's kernels executed under oracle/ti_shim on the inputs of tests/golden/kat_hand.json
    (frexp_bit, morton3D, packbits, the hash encoder on every hash KAT, the training composite) -- what tests/test_kat_hand.py holds
    against the hand-derived answers;
  * tests/golden/ref_driver_shape.json: data the drop-in tests compare this package with -- the parameter names of the reference's
    public callables (tests/test_dropin_imports.py), the ordered boundary calls of train.py's training iteration, setup and
    evaluation loop, and the line similarity of examples/train_reference_shape.py with train.py together with the example's sha256
    (tests/test_reference_shape.py).  No source text, and nothing per line of it, is stored.
Where the checkout exists the tests recompute both and require them to equal these files.  TEST INFRASTRUCTURE ONLY."""
import importlib.util
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TESTS = os.path.join(ROOT, "tests")
OUT = os.path.join(TESTS, "golden")
SHIM_NPZ = os.path.join(OUT, "ref_kat_shim.npz")
DRIVER_JSON = os.path.join(OUT, "ref_driver_shape.json")


def _test_module(name):
    for p in (TESTS, HERE, ROOT, os.path.join(ROOT, "taichi-nerfs_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    spec = importlib.util.spec_from_file_location(name, os.path.join(TESTS, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def shim_kat_outputs(R):
    """The reference's kernels (R = gen_golden.load_reference()) on the KAT inputs of tests/test_kat_hand.py."""
    import torch
    K = _test_module("test_kat_hand")
    import taichi as ti                                            # (the shim; put on sys.path by load_reference)
    U, kat, out = R["utils"], K.KAT, {}
    out["frexp_bit"] = np.array([int(U.frexp_bit(ti.f32(x))) for x, _ in kat["frexp_bit"]["cases"]], np.int64)
    pts = torch.tensor([c for c, _ in kat["morton3d"]["cases"]], dtype=torch.int32)
    idx = torch.zeros(len(pts), dtype=torch.int32)
    U.morton3D_kernel(pts, idx)
    out["morton3d"] = idx.numpy().astype(np.int64)
    bits = torch.zeros(1, dtype=torch.uint8)
    U.packbits(torch.tensor(kat["packbits"]["grid"], dtype=torch.float32), kat["packbits"]["threshold"], bits)
    out["packbits"] = bits.numpy().astype(np.int64)
    enc = R["hash_encoder"].HashEncoder(max_params=2**19, levels=16, base_res=16.0, max_res=1024.0, feature_per_level=2)
    for name, x, table, _, _, _ in K._hash_cases():
        o = torch.zeros(1, 32)
        enc._hash_encoder_kernel(torch.from_numpy(x), torch.from_numpy(table), o, enc.hash_map_sizes, enc.offsets, 1)
        out["hash__" + name] = o.numpy()
    s, c, dl, t, ra, thr, _ = K._composite_inputs()
    n, S = ra.shape[0], s.shape[0]
    total = torch.zeros(n, dtype=torch.int32); op = torch.zeros(n); dep = torch.zeros(n); rgb = torch.zeros(n, 3)
    ws = torch.full((S,), float("nan")); T = torch.zeros(S + 1)
    # (argument order of volume_train.py:7-20)
    R["volume_train"].volume_rendering_kernel(torch.from_numpy(s), torch.from_numpy(c), torch.from_numpy(dl), torch.from_numpy(t),
                                              torch.from_numpy(ra), thr, T, total, op, dep, rgb, ws)
    out.update(composite_total=total.numpy(), composite_opacity=op.numpy(), composite_depth=dep.numpy(), composite_rgb=rgb.numpy(),
               composite_ws=ws.numpy())
    return out


def driver_shape(ref_root):
    shape = _test_module("test_reference_shape")
    return {"signatures": _test_module("test_dropin_imports").reference_signatures(ref_root),
            "train_py": shape.driver_structure(os.path.join(ref_root, "train.py")),
            "example_vs_train_py": shape.example_similarity(os.path.join(ref_root, "train.py"))}


def main():
    from gen_golden import REF, load_reference
    np.savez_compressed(SHIM_NPZ, **shim_kat_outputs(load_reference()))
    with open(DRIVER_JSON, "w") as f:
        json.dump(driver_shape(REF), f, indent=1)
        f.write("\n")
    print("wrote", SHIM_NPZ, DRIVER_JSON)


if __name__ == "__main__":
    main()
