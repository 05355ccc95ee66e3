"""ctypes binding of libngp_hip.so (C ABI declared in include/ngp_hip.h).

This is the binding a maintainer of the reference would add in place of Taichi's torch interop: every
`@ti.kernel` launch in the reference's modules/*.py becomes one call through this table with
`tensor.data_ptr()` + the current torch stream.  There is NO fallback: if the shared library is missing or
fails to load, `load()` raises -- the product path never routes through a CPU implementation.

The table is not written here: argument types, result types, struct layouts and constants are read out of the two
headers when this module is imported (ngp_hip/cabi.py), so the headers are the one definition of the ABI.
"""
import ctypes
import glob
import os
import shutil
import subprocess

from . import cabi

_HERE = os.path.dirname(os.path.abspath(__file__))
PKG_ROOT = os.path.dirname(_HERE)
CSRC = os.path.join(PKG_ROOT, "csrc")
INCLUDE = os.path.join(os.path.dirname(PKG_ROOT), "include")
LIB_PATH = os.path.join(CSRC, "libngp_hip.so")
SOURCES = ["march.hip", "hash_grid.hip", "hash_bwd_lds.hip", "composite.hip", "sh_grid.hip", "mlp.hip", "optim.hip", "distortion.hip", "occupancy.hip", "rays.hip",
           "render.hip", "exchange.hip", "triplane.hip", "voxel_grid.hip", "deploy.hip", "hash_grad_input.hip", "hash_grad_input2.hip", "mesh.hip",
           "ray_grad.hip", "surface.hip", "resample.hip", "sdf_trace.hip", "mesh_sdf.hip", "mesh_raycast.hip", "mesh_winding.hip",
           "mesh_components.hip", "mesh_simplify.hip", "mesh_smooth.hip", "mesh_color.hip"]
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared"]
FLAGS_STAMP = LIB_PATH + ".flags"      # the flags the in-tree .so was built with: a flag change rebuilds
ABI_HEADERS = [os.path.join(INCLUDE, "ngp_hip.h"), os.path.join(INCLUDE, "ngp_hip_experimental.h")]


def _read_headers():
    """The two headers, parsed (once per process: at import).  The second sees the first's #defines."""
    out = []
    for path in ABI_HEADERS:
        if not os.path.exists(path):
            raise RuntimeError("%s is missing: libngp_hip.so cannot be bound without the header that declares it. "
                               "There is no CPU fallback." % path)
        with open(path) as f:
            out.append(cabi.parse(f.read(), out[0].defines if out else None))
    return out


_ABI, _ABI_EXPERIMENTAL = _read_headers()
NGP_MAX_LEVELS = _ABI.defines["NGP_MAX_LEVELS"]
ABI_VERSION = _ABI.defines["NGP_ABI_VERSION"]
BWD_PLAN_DETERMINISTIC, BWD_PLAN_CONCENTRATED = _ABI.defines["NGP_BWD_PLAN_DETERMINISTIC"], _ABI.defines["NGP_BWD_PLAN_CONCENTRATED"]


class HashLevels(ctypes.Structure):
    """`ngp_hash_levels` (include/ngp_hip.h)."""
    _fields_ = _ABI.structs["ngp_hash_levels"]

    def with_plan(self, bits):
        """A copy of this level table whose LDS-sliced scatter-add runs on the task plan `bits` (BWD_PLAN_*); copies are cached."""
        bits = int(bits)
        if bits == self.bwd_plan:
            return self
        cache = self.__dict__.setdefault("_plans", {})
        lv = cache.get(bits)
        if lv is None:
            lv = HashLevels()
            ctypes.memmove(ctypes.byref(lv), ctypes.byref(self), ctypes.sizeof(HashLevels))
            lv.bwd_plan = bits
            cache[bits] = lv
        return lv


class TriPlaneLevels(ctypes.Structure):
    """`ngp_triplane_levels` (include/ngp_hip.h)."""
    _fields_ = _ABI.structs["ngp_triplane_levels"]


class RenderArgs(ctypes.Structure):
    """`ngp_render_args` (include/ngp_hip.h): the argument block of ngp_render_train_fwd / _bwd."""
    _fields_ = _ABI.structs["ngp_render_args"]


def _sources():
    return [os.path.join(CSRC, s) for s in SOURCES if os.path.exists(os.path.join(CSRC, s))]


def _flags():
    return HIPCC_FLAGS + os.environ.get("NGP_HIPCC_EXTRA", "").split()   # e.g. -DNGP_BWD_DIAG for the timing experiments in profiles/microbench


def needs_build():
    if not os.path.exists(LIB_PATH):
        return True
    t = os.path.getmtime(LIB_PATH)
    deps = _sources() + glob.glob(os.path.join(CSRC, "*.h")) + ABI_HEADERS      # every device header: none to remember by hand
    if any(os.path.getmtime(d) > t for d in deps if os.path.exists(d)):
        return True
    # a library built with other flags (a -D... diagnostic build left in the tree) is stale too; no stamp = a prebuilt library that
    # travelled without one: trusted when no extra flags are asked for
    if os.path.exists(FLAGS_STAMP):
        return open(FLAGS_STAMP).read().split() != _flags()
    return bool(os.environ.get("NGP_HIPCC_EXTRA", "").split())


def build(force=False, verbose=False):
    """Cross-compile every HIP source for gfx950 into the in-tree libngp_hip.so (works without a GPU)."""
    if not force and not needs_build():
        return LIB_PATH
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        raise RuntimeError("hipcc not found: cannot build libngp_hip.so")
    tmp = LIB_PATH + ".tmp.%d" % os.getpid()
    cmd = [hipcc] + _flags() + ["-o", tmp] + _sources()
    if verbose:
        print(" ".join(cmd))
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError("hipcc failed:\n" + res.stdout + res.stderr)
    os.replace(tmp, LIB_PATH)
    with open(FLAGS_STAMP, "w") as f:
        f.write(" ".join(_flags()))
    return LIB_PATH


# The binding, derived: a scalar by its C type, `ngp_hash_levels*` / `ngp_triplane_levels*` as typed pointers, every other pointer
# (ngp_render_args* included: callers pass byref) as c_void_p, the result type as the prototype states it.
_BOUND = cabi.bind({**_ABI.functions, **_ABI_EXPERIMENTAL.functions},
                   {"ngp_hash_levels": ctypes.POINTER(HashLevels), "ngp_triplane_levels": ctypes.POINTER(TriPlaneLevels),
                    "ngp_render_args": ctypes.c_void_p})
SIGNATURES = {name: argtypes for name, (_, argtypes) in _BOUND.items()}        # name -> argtypes
RESTYPES = {name: restype for name, (restype, _) in _BOUND.items()}            # name -> restype (int status, or a long long byte count)
# declared in include/ngp_hip_experimental.h: exported and typed like the rest, called by no default path of the package
EXPERIMENTAL = set(_ABI_EXPERIMENTAL.functions)
_lib = None


def load():
    """Load libngp_hip.so (after torch, so both share torch's libamdhip64.so.7) and type every entry point."""
    global _lib
    if _lib is not None:
        return _lib
    import torch  # noqa: F401  (must be imported first: the HIP runtime SONAME is then already resolved)
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "libngp_hip.so is not built (%s). Run `python __graft_entry__.py` or "
            "`python -c 'import __graft_entry__ as g; g.build()'`. There is no CPU fallback." % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
    for name, argtypes in SIGNATURES.items():
        fn = getattr(lib, name)     # AttributeError here = header/library mismatch: fail loudly
        fn.argtypes = argtypes
        fn.restype = RESTYPES[name]
    if lib.ngp_abi_version() != ABI_VERSION:     # a prebuilt library that travelled with other headers: the derived argtypes could be wrong
        raise RuntimeError("%s reports ABI version %d, but include/ngp_hip.h declares %d: rebuild the library from this tree "
                           "(`python __graft_entry__.py`). There is no CPU fallback." % (LIB_PATH, lib.ngp_abi_version(), ABI_VERSION))
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        raise RuntimeError("%s failed with code %d (negated hipError_t, or -1 for bad arguments)" % (what, rc))
