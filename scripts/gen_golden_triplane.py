"""Generate tests/golden/ref_triplane.npz by executing the reference's UNMODIFIED modules/triplane.py (kernel + autograd glue)
under oracle/ti_shim.  Needs a reference checkout (the path oracle/gen_golden.py names, or REF=...):
    python scripts/gen_golden_triplane.py
The tests read only the .npz; the table is regenerated there from oracle.gen_golden.golden_table (not stored).

Static-loop scoping: the reference kernel reuses `i` as a `ti.static` loop target (triplane.py:80) inside the ndrange loop over `i`.
Taichi scopes static-loop targets, so :98 writes row i; the shim runs kernel bodies as plain Python, where the inner loop would
overwrite `i`.  This script gives the shim that scoping (the shim itself stays as it is): while the reference module is loaded,
a `for NAME in ti.static(...)` nested in a loop over NAME gets its target renamed within its own body.
Recorded: the forward, the Taichi-level gradient (kernel.grad with a non-leaf table: d table exactly once) and the module-level
gradient (the leaf nn.Parameter: 2x, because the glue returns the parameter's own .grad) sparsely; the reference NGP's state_dict."""
import ast
import hashlib
import importlib
import json
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import gen_golden  # noqa: E402
from oracle.gen_golden import OUT, golden_table  # noqa: E402

REF = os.environ.get("REF", gen_golden.REF)


class _ScopeStaticTargets(ast.NodeTransformer):
    """`for i in ti.static(...)` inside a loop whose target binds `i`: rename the inner target (and its uses in the inner body)."""

    def __init__(self):
        self.bound, self.n = [], 0

    @staticmethod
    def _names(t):
        return {n.id for n in ast.walk(t) if isinstance(n, ast.Name)}

    def visit_For(self, node):
        inner_static = (isinstance(node.iter, ast.Call) and isinstance(node.iter.func, ast.Attribute) and node.iter.func.attr == "static"
                        and isinstance(node.target, ast.Name))
        if inner_static and any(node.target.id in b for b in self.bound):
            old, new = node.target.id, "%s__static%d" % (node.target.id, self.n)
            self.n += 1
            for sub in ast.walk(ast.Module(body=node.body, type_ignores=[])):
                if isinstance(sub, ast.Name) and sub.id == old:
                    sub.id = new
            node.target.id = new
        self.bound.append(self._names(node.target))
        self.generic_visit(node)
        self.bound.pop()
        return node


def load_triplane():
    sys.path.insert(0, os.path.join(gen_golden.HERE, "ti_shim"))
    import taichi as ti_shim
    base = ti_shim._Rewrite

    class _Rewrite(base):
        def visit_FunctionDef(self, node):
            node = _ScopeStaticTargets().visit(node)
            self.generic_visit(node)
            return node

    ti_shim._Rewrite = _Rewrite
    gen_golden.REF = REF
    gen_golden.load_reference()                      # registers the `refmodules` package over REF/modules
    return importlib.import_module("refmodules.triplane"), ti_shim


def reference_state_dict_shapes():
    """Keys and shapes of the reference's NGP(scale=0.5, pos_encoder_type='triplane', max_res=1024) (networks.py:101-107)."""
    sys.path.insert(0, os.path.join(ROOT, "taichi-nerfs_amd", "compat"))     # kornia's create_meshgrid3d
    for name in ("rendering", "sh_utils", "networks"):
        try:
            importlib.import_module("refmodules." + name)
        except Exception as e:  # noqa: BLE001
            raise RuntimeError("cannot import the reference's networks.py under the shim: %r" % e)
    ngp = sys.modules["refmodules.networks"].NGP(scale=0.5, pos_encoder_type="triplane", max_res=1024)   # train.py at scale 0.5
    return {k: list(v.shape) for k, v in ngp.state_dict().items()}


def points(rng, n, max_res, res_top):
    x = rng.random((n, 3), dtype=np.float32)
    x[:8] = [[0, 0, 0], [1, 1, 1], [0.5, 0.5, 0.5], [1, 0, 0.5], [0, 1, 1], [0.999999, 1e-7, 0.5], [0.3, 1.0, 0.0], [0.25, 0.75, 1.0]]
    # the top-level collision: grid points 0 and 1 of the top level map to one full-resolution entry (max_res 1024: x < 1.5 / 1023)
    g = 1.0 / (res_top - 1)
    x[8:14] = [[0.2 * g, 0.3 * g, 0.1 * g], [0.9 * g, 0.5, 0.4 * g], [0.6 * g, 0.6 * g, 0.6 * g], [0.5, 0.1 * g, 0.7],
               [1.2 * g, 0.3, 0.95 * g], [0.0, 0.45 * g, 0.5]]
    x[14:22] = x[22:30] + rng.normal(0, 2e-4, (8, 3)).astype(np.float32)        # near-duplicates: shared cells on every level
    return np.clip(x, 0, 1).astype(np.float32)


def main():
    warnings.filterwarnings("ignore", message="The .grad attribute of a Tensor that is not a leaf")
    tri, ti_shim = load_triplane()
    rng = np.random.default_rng(515)
    T = torch.from_numpy
    data = {}
    for max_res in (64, 1024):
        enc = tri.TriPlaneEncoder(base_res=16, max_res=max_res, levels=8, feature_per_level=4)
        table = golden_table(enc.total_param_size)
        log_b = np.float32(enc.log_b)
        res = np.array([np.uint32(np.ceil(np.float32(16) * ti_shim.exp(np.float32(l) * log_b) - np.float32(1.0))) + 1 for l in range(8)],
                       dtype=np.uint32)
        n = 56
        x = points(rng, n, max_res, int(res[-1]))
        dout = rng.normal(0, 1, (n, 32)).astype(np.float32)
        dout[30:34] = 0.0
        # (1) Taichi level: kernel.grad with a non-leaf table -> d table exactly once
        tab = T(table.copy()).requires_grad_(True)
        params = tab * 1.0
        out = enc._module_function(T(x), params)
        out.backward(T(dout))
        g1 = tab.grad.numpy().copy()
        # (2) through the module as networks.py uses it (leaf nn.Parameter): the glue's factor 2
        with torch.no_grad():
            enc.plane_embedding.copy_(T(table))
        enc.plane_embedding.grad = None
        out2 = enc(T(x))
        out2.backward(T(dout))
        g2 = enc.plane_embedding.grad.numpy().copy()
        nz = np.flatnonzero((g1 != 0) | (g2 != 0))
        tag = "r%d" % max_res
        data.update({tag + "_x": x, tag + "_dout": dout, tag + "_out": out.detach().numpy().copy(), tag + "_res": res,
                     tag + "_grad_idx": nz.astype(np.int64), tag + "_grad_taichi": g1[nz], tag + "_grad_module": g2[nz],
                     tag + "_log_b": np.float64(enc.log_b), tag + "_total_param_size": np.int64(enc.total_param_size)})
        assert np.array_equal(out.detach().numpy(), out2.detach().numpy())
        print("max_res %d: res %s, %d gradient entries, |out| max %.3g" % (max_res, res.tolist(), len(nz), np.abs(data[tag + "_out"]).max()))
    shapes = reference_state_dict_shapes()
    data["state_dict_json"] = np.array(json.dumps(shapes, sort_keys=True))
    path = os.path.join(OUT, "ref_triplane.npz")
    np.savez_compressed(path, **data)
    print("wrote", path, os.path.getsize(path), "bytes")
    src = os.path.join(REF, "modules", "triplane.py")
    print("sha256 triplane.py", hashlib.sha256(open(src, "rb").read()).hexdigest())
    print("sha256 ref_triplane.npz", hashlib.sha256(open(path, "rb").read()).hexdigest())


if __name__ == "__main__":
    main()
