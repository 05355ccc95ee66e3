"""The C-ABI library builds for gfx950, loads, and exports exactly what include/ngp_hip.h declares
(no compute calls: there is no GPU in the CPU test tier)."""
import ctypes
import os
import re

import pytest

from conftest import ROOT


def _declared(name="ngp_hip.h"):
    hdr = open(os.path.join(ROOT, "include", name)).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return sorted(set(re.findall(r"\b(?:int|long long)\s+(ngp_[a-z0-9_]+)\s*\(", hdr)))


def test_header_symbols_exported(hip_lib):
    """The boundary header and the experimental header are disjoint, together they are exactly what the ctypes table binds, and the
    library exports every one of them."""
    from ngp_hip import lib
    names, extra = _declared(), _declared("ngp_hip_experimental.h")
    assert len(names) >= 19 and not set(names) & set(extra)
    for n in names + extra:
        assert hasattr(hip_lib, n), "libngp_hip.so does not export %s" % n
    assert sorted(lib.SIGNATURES) == sorted(names + extra), "ngp_hip/lib.py binds a different symbol set than the headers declare"
    assert sorted(lib.EXPERIMENTAL) == extra
    assert hip_lib.ngp_abi_version() == 3


def test_no_default_path_calls_an_experimental_entry_point():
    """Round 6: what include/ngp_hip_experimental.h declares is reached only through a non-default switch, a test or a
    diagnostic.  The drop-in surface (modules/, compat/), the operator layer and the fused render never name one; FusedTrainer names exactly
    the two that sit behind switches that are off by default (NGP_EXPERIMENT comm_overlap=1, `_fold_prologue = False`);
    ngp_hip/p2p.py (reached only through FusedTrainer(exchange="p2p")) names the three of the direct exchange."""
    from ngp_hip import lib
    pkg = os.path.join(ROOT, "taichi-nerfs_amd")
    hits = {}
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py") and f != "lib.py" or f == "render.hip":
                src = open(os.path.join(dp, f)).read()
                for n in lib.EXPERIMENTAL:
                    if re.search(r"\b%s\b" % n, src):
                        hits.setdefault(os.path.relpath(os.path.join(dp, f), pkg), set()).add(n)
    assert hits == {os.path.join("ngp_hip", "trainer.py"): {"ngp_hash_bwd_sliced_main_adam", "ngp_hash_bwd_sliced_main_levels"},
                    # the direct peer-memory exchange (FusedTrainer(exchange="p2p"), a prototype: default "rccl")
                    os.path.join("ngp_hip", "p2p.py"): {"ngp_p2p_max_peers", "ngp_p2p_push", "ngp_p2p_wait"}}, hits


def _gcc_layout(tmp_path, struct, names, extra=""):
    """[sizeof(struct), offsetof(struct, n) for n in names, *the integers `extra` prints] as gcc lays include/ngp_hip.h out."""
    import subprocess
    src = tmp_path / (struct + ".c")
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void) {\n  printf("%%zu\\n", sizeof(%s));\n%s%s  return 0;\n}\n'
                   % (os.path.join(ROOT, "include", "ngp_hip.h"), struct,
                      "".join('  printf("%%zu\\n", offsetof(%s, %s));\n' % (struct, n) for n in names), extra))
    exe = tmp_path / struct
    subprocess.run(["gcc", "-o", str(exe), str(src)], check=True)
    return [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]


def test_struct_layout_matches_header(tmp_path):
    """ngp_hash_levels: the ctypes structure has gcc's layout of include/ngp_hip.h, field by field (round 6: + bwd_plan, the scatter-add's
    task-plan bits that used to be per-thread state of the library)."""
    from ngp_hip import lib
    from ngp_hip.lib import HashLevels
    names = [f[0] for f in HashLevels._fields_]
    assert names[-1] == "bwd_plan"
    out = _gcc_layout(tmp_path, "ngp_hash_levels", names, '  printf("%u %u\\n", NGP_BWD_PLAN_DETERMINISTIC, NGP_BWD_PLAN_CONCENTRATED);\n')
    assert out[0] == ctypes.sizeof(HashLevels) == 16 + 4 * 16 * 4 + 4
    assert out[1:-2] == [getattr(HashLevels, n).offset for n in names]
    assert out[-2:] == [lib.BWD_PLAN_DETERMINISTIC, lib.BWD_PLAN_CONCENTRATED]


def test_triplane_levels_layout_matches_header(tmp_path):
    """ngp_triplane_levels: size and every field's offset and size are gcc's."""
    from ngp_hip.lib import TriPlaneLevels
    names = [f[0] for f in TriPlaneLevels._fields_]
    assert names == ["n_levels", "n_features", "max_res", "reserved", "scale", "resolution"]
    out = _gcc_layout(tmp_path, "ngp_triplane_levels", names,
                      "".join('  printf("%%zu\\n", sizeof(((ngp_triplane_levels*)0)->%s));\n' % n for n in names))
    assert out[0] == ctypes.sizeof(TriPlaneLevels) == 16 + 2 * 16 * 4
    assert out[1:1 + len(names)] == [getattr(TriPlaneLevels, n).offset for n in names]
    assert out[1 + len(names):] == [getattr(TriPlaneLevels, n).size for n in names]


def test_render_args_layout_matches_header(tmp_path):
    """ngp_render_args (the argument block of ngp_render_train_fwd / _bwd): the ctypes structure has the C compiler's layout -- every field
    at the offset gcc gives it in include/ngp_hip.h."""
    from ngp_hip.lib import RenderArgs
    names = [f[0] for f in RenderArgs._fields_]
    assert len(names) == 61
    out = _gcc_layout(tmp_path, "ngp_render_args", names)
    assert out[0] == ctypes.sizeof(RenderArgs)
    assert out[1:] == [getattr(RenderArgs, n).offset for n in names]


_C_SCALAR = {ctypes.c_int: "int", ctypes.c_uint: "unsigned int", ctypes.c_longlong: "long long", ctypes.c_ulonglong: "unsigned long long",
             ctypes.c_float: "float", ctypes.c_double: "double"}
_C_STRUCT = {"HashLevels": "ngp_hash_levels", "TriPlaneLevels": "ngp_triplane_levels"}


def _abi_check_source(signatures, restypes):
    """A C++ translation unit that compiles iff every entry of the ctypes table agrees with its prototype: one static_assert per arity,
    result and argument.  Scalars must be the same type; a pointer must be a pointer, a typed struct pointer one to that struct."""
    def claim(t, expr, what):
        if t in _C_SCALAR:
            cond = "std::is_same<%s, %s>::value" % (expr, _C_SCALAR[t])
        elif t is ctypes.c_void_p:
            cond = "std::is_pointer<%s>::value" % expr
        elif issubclass(t, ctypes._Pointer) and t._type_.__name__ in _C_STRUCT:
            cond = "std::is_same<std::remove_cv_t<std::remove_pointer_t<%s>>, %s>::value" % (expr, _C_STRUCT[t._type_.__name__])
        else:
            raise AssertionError("%s: the table holds %r, which this check cannot state in C++" % (what, t))
        return 'static_assert(%s, "%s");\n' % (cond, what)
    out = ['#include <tuple>\n#include <type_traits>\n#include "ngp_hip.h"\n#include "ngp_hip_experimental.h"\n'
           "template <class F> struct sig;\n"
           "template <class R, class... A> struct sig<R (*)(A...)> {\n"
           "    using result = R;\n    static constexpr int arity = sizeof...(A);\n"
           "    template <int I> using arg = std::tuple_element_t<I, std::tuple<A...>>;\n};\n"]
    for name, argtypes in signatures.items():
        s = "sig<decltype(&%s)>" % name
        out.append('static_assert(%s::arity == %d, "%s: arity");\n' % (s, len(argtypes), name))
        out.append(claim(restypes[name], s + "::result", name + ": result"))
        out += [claim(t, "%s::arg<%d>" % (s, i), "%s: argument %d" % (name, i)) for i, t in enumerate(argtypes)]
    return "".join(out)


def _syntax_check(tmp_path, name, source):
    import subprocess
    src = tmp_path / name
    src.write_text(source)
    return subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)


def test_compiler_agrees_with_every_signature(tmp_path):
    """The C++ compiler holds the whole derived table -- arity, result type and every argument of all entry points -- against the
    prototypes of the two headers; and it does refuse a table with one scalar changed, naming the entry."""
    from ngp_hip import lib
    assert len(lib.SIGNATURES) >= 140 and set(lib.RESTYPES) == set(lib.SIGNATURES)
    source = _abi_check_source(lib.SIGNATURES, lib.RESTYPES)
    assert source.count("static_assert") == sum(2 + len(a) for a in lib.SIGNATURES.values())
    res = _syntax_check(tmp_path, "abi_check.cpp", source)
    assert res.returncode == 0, res.stderr[-4000:]
    # negative control: ngp_ray_aabb(const float*, const float*, float scale, int, float*, void*) with `scale` typed as an int
    wrong = {k: list(v) for k, v in lib.SIGNATURES.items()}
    assert wrong["ngp_ray_aabb"][2] is ctypes.c_float
    wrong["ngp_ray_aabb"][2] = ctypes.c_int
    res = _syntax_check(tmp_path, "abi_wrong.cpp", _abi_check_source(wrong, lib.RESTYPES))
    assert res.returncode != 0 and "ngp_ray_aabb: argument 2" in res.stderr
    assert res.stderr.count("static assertion failed") == 1, res.stderr[-4000:]
    # ... and a long long result typed as the int every status returns
    wrong_res = dict(lib.RESTYPES, ngp_mesh_workspace_bytes=ctypes.c_int)
    res = _syntax_check(tmp_path, "abi_wrong_result.cpp", _abi_check_source(lib.SIGNATURES, wrong_res))
    assert res.returncode != 0 and "ngp_mesh_workspace_bytes: result" in res.stderr


_EDGE_HEADER = """
/* int ngp_in_a_comment(float x); is not a prototype:
 * long long ngp_nor_this(void);
 */
#ifndef EDGE_H
#define EDGE_H
#ifdef __cplusplus
extern "C" {
#endif
#define NGP_MAX_LEVELS 16
#define NGP_SOME_BITS 2u
typedef struct ngp_edge {
    int32_t a /*x*/, b;
    const float* w[5]; /* five matrices */
    float s[NGP_MAX_LEVELS];
    long long cap;
} ngp_edge;
int ngp_nothing(void);
int ngp_spread(const float* xyzs /*[n,3]*/,
               const ngp_hash_levels* lv, /* int ngp_in_a_comment2(int n); */
               int n /*[n,3]*/, float* out /*[n, L*F]*/,
               void* stream);
long long ngp_kinds(unsigned long long seed, unsigned int mask, float* const* p, void** event, double d, uint32_t u, long long n,
                    const ngp_edge* e);
#ifdef __cplusplus
}
#endif
#endif
"""


def test_header_parser_edge_cases():
    """ngp_hip/cabi.py on literal header text: comments go first, declarators of every kind the headers use map as documented, and what
    it does not understand raises with the name of the entry point or struct."""
    from ngp_hip import cabi
    h = cabi.parse(_EDGE_HEADER)
    assert h.defines == {"NGP_MAX_LEVELS": 16, "NGP_SOME_BITS": 2}                      # not the include guard
    assert sorted(h.functions) == ["ngp_kinds", "ngp_nothing", "ngp_spread"]          # nothing from inside a comment
    assert h.structs == {"ngp_edge": [("a", ctypes.c_int32), ("b", ctypes.c_int32), ("w", ctypes.c_void_p * 5),
                                      ("s", ctypes.c_float * 16), ("cap", ctypes.c_longlong)]}

    class Levels(ctypes.Structure):
        _fields_ = [("n", ctypes.c_int)]
    P, LV = ctypes.c_void_p, ctypes.POINTER(Levels)
    bound = cabi.bind(h.functions, {"ngp_hash_levels": LV, "ngp_edge": P})
    assert bound["ngp_nothing"] == (ctypes.c_int, [])
    assert bound["ngp_spread"] == (ctypes.c_int, [P, LV, ctypes.c_int, P, P])
    assert bound["ngp_kinds"] == (ctypes.c_longlong, [ctypes.c_ulonglong, ctypes.c_uint, P, P, ctypes.c_double, ctypes.c_uint32,
                                                      ctypes.c_longlong, P])
    with pytest.raises(cabi.HeaderError, match="ngp_spread.*ngp_hash_levels"):          # a pointer to something nobody declared
        cabi.bind(h.functions, {})

    bad = cabi.parse("int ngp_sized(const float* x, size_t n, void* stream);")
    with pytest.raises(cabi.HeaderError, match=r"ngp_sized.*size_t n"):
        cabi.bind(bad.functions, {})
    with pytest.raises(cabi.HeaderError, match=r"ngp_cb"):                              # a function pointer: not understood, not guessed
        cabi.parse("int ngp_cb(void (*f)(int), void* stream);")
    with pytest.raises(cabi.HeaderError, match=r"struct ngp_s.*size_t n"):
        cabi.parse("typedef struct ngp_s { int32_t a; size_t n; } ngp_s;")
    with pytest.raises(cabi.HeaderError, match=r"struct ngp_s.*NGP_UNKNOWN"):
        cabi.parse("typedef struct ngp_s { float s[NGP_UNKNOWN]; } ngp_s;")
    assert cabi.parse("typedef struct ngp_s { float s[N]; } ngp_s;", {"N": 3}).structs["ngp_s"] == [("s", ctypes.c_float * 3)]


def test_missing_header_fails_loudly(monkeypatch, tmp_path):
    from ngp_hip import lib
    monkeypatch.setattr(lib, "ABI_HEADERS", [str(tmp_path / "ngp_hip.h")])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lib._read_headers()


def test_abi_version_mismatch_fails_loudly(hip_lib, monkeypatch):
    """A library whose ngp_abi_version() is not the headers' NGP_ABI_VERSION is refused: its argument lists may not be the derived ones."""
    from ngp_hip import lib
    assert lib.ABI_VERSION == hip_lib.ngp_abi_version()
    monkeypatch.setattr(lib, "_lib", None)
    monkeypatch.setattr(lib, "ABI_VERSION", lib.ABI_VERSION + 1)
    with pytest.raises(RuntimeError, match="ABI version"):
        lib.load()
    assert lib._lib is None


def test_ops_refuse_cpu_tensors(hip_lib):
    """The product path has no CPU fallback: host tensors are rejected loudly."""
    import torch
    from ngp_hip import ops
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.ray_aabb(torch.zeros(4, 3), torch.ones(4, 3), 0.5)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.sh16_fwd(torch.zeros(4, 3))


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    from ngp_hip import lib
    monkeypatch.setattr(lib, "_lib", None)
    monkeypatch.setattr(lib, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lib.load()


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "taichi-nerfs_amd")
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                src = open(os.path.join(dp, f)).read()
                assert "oracle" not in src.replace("the CPU oracle", "").replace("against the oracle", "") \
                    .replace("the oracle", ""), "%s mentions the oracle" % f
