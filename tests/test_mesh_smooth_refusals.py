"""The smoothing entries of the C ABI refuse what their contract excludes with -1 BEFORE anything is launched (include/ngp_hip.h,
"mesh smoothing"), so the refusals can be checked without a GPU: every pointer below is a made-up address that is never followed."""
import ctypes
import math

P = ctypes.c_void_p(4096)            # "not null": a refused call does not touch it
NULL = ctypes.c_void_p(0)
INF = float("inf")


def _move(*v):
    return (ctypes.c_float * 3)(*v)


def _smooth(lib, x_a=P, x_b=ctypes.c_void_p(8192), x0=ctypes.c_void_p(12288), row_start=P, neighbours=P, multiplicity=P, flags=P, fixed=NULL,
            n_vertices=10, n_slots=60, iterations=1, lam=0.5, mu=-0.53, mode=0, max_move=(INF, INF, INF)):
    return lib.ngp_mesh_smooth(x_a, x_b, x0, row_start, neighbours, multiplicity, flags, fixed, n_vertices, n_slots, iterations, lam, mu, mode,
                               _move(*max_move) if max_move is not None else NULL, NULL)


def test_smooth_refuses_bad_arguments(hip_lib):
    lib = hip_lib
    for name in ("x_a", "x_b", "row_start", "neighbours", "multiplicity", "flags"):
        assert _smooth(lib, **{name: NULL}) == -1, name
    assert _smooth(lib, max_move=None) == -1
    assert _smooth(lib, x_b=P) == -1                                               # ping-pong: the two buffers must differ
    assert _smooth(lib, n_vertices=0) == -1 and _smooth(lib, n_slots=-1) == -1 and _smooth(lib, n_slots=2**31) == -1
    assert _smooth(lib, iterations=-1) == -1
    for bad in (math.nan, INF, -INF):
        assert _smooth(lib, lam=bad) == -1 and _smooth(lib, mu=bad) == -1
    for bad in ((-1e-9, 1.0, 1.0), (1.0, math.nan, 1.0), (1.0, 1.0, -INF)):
        assert _smooth(lib, max_move=bad) == -1, bad
    assert _smooth(lib, mode=3) == -1 and _smooth(lib, mode=-1) == -1
    assert _smooth(lib, max_move=(0.5, INF, INF), x0=NULL) == -1                   # a bound needs the original positions ...
    assert _smooth(lib, max_move=(0.5, INF, INF), x0=P) == -1                      # ... in a buffer of their own


def test_adjacency_and_normals_refuse_bad_sizes(hip_lib):
    lib = hip_lib
    too_many = (2**31 - 1) // 6 + 1                                                # 6 T would pass 2^31 - 1
    assert lib.ngp_mesh_adjacency_bytes(0) == -1 and lib.ngp_mesh_adjacency_bytes(too_many) == -1
    assert lib.ngp_mesh_adjacency_bytes(too_many - 1) > 0 and lib.ngp_mesh_adjacency_bytes(1) >= 6 * 4 + 6 + 4
    for T, V in ((0, 5), (5, 0), (-1, 5), (too_many, 5)):
        assert lib.ngp_mesh_adjacency_keys(P, T, V, P, P, NULL) == -1
        assert lib.ngp_mesh_adjacency_build(P, T, V, P, P, P, P, P, P, P, NULL) == -1
        assert lib.ngp_mesh_vertex_normals_keys(P, T, V, P, NULL) == -1
        assert lib.ngp_mesh_vertex_normals(P, P, T, V, P, P, P, NULL) == -1
    assert lib.ngp_mesh_adjacency_keys(NULL, 5, 5, P, P, NULL) == -1 and lib.ngp_mesh_adjacency_keys(P, 5, 5, NULL, P, NULL) == -1
    assert lib.ngp_mesh_adjacency_build(P, 5, 5, P, NULL, P, P, P, P, P, NULL) == -1
    assert lib.ngp_mesh_vertex_normals(P, P, 5, 5, P, P, NULL, NULL) == -1


def test_python_surface_refuses_before_the_device(hip_lib):
    """Host tensors, a wrong boundary mode and a pass band outside (0, 1 / lam) are errors of the caller, raised as such."""
    import pytest
    import torch
    import ngp_hip
    v, f = torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ngp_hip.adjacency((v, f))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ngp_hip.vertex_normals(v, f)
    with pytest.raises(ValueError):
        ngp_hip.taubin_mu(0.5, pass_band=2.5)
    assert abs(ngp_hip.taubin_mu(0.5) - 1.0 / (0.1 - 2.0)) < 1e-15
