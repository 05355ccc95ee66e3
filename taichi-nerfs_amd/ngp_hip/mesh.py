"""Isosurface meshes from the models: sample a scalar field on a regular grid, run marching tetrahedra on the device
(csrc/mesh.hip through ops.mesh_count / ops.mesh_emit), write the result as .ply or .obj.

    mesh = extract_mesh(model, resolution=256, threshold=0.01 * 1024 / 3**0.5)        # NGP (any encoder) or VoxelGrid
    mesh = extract_mesh(sdf_fn, 128, 0.0, bounds=((0, 0, 0), (1, 1, 1)), sign=-1)      # any callable points [n,3] -> values [n]
    write_ply("scene.ply", mesh)

The mesh is indexed (shared vertices), deterministic (the same grid gives the same bytes) and, wherever the surface stays off the grid
boundary, a closed consistently oriented 2-manifold; the exact contract is in DESIGN.md section 3.  The extraction itself costs one host
read (the vertex and face counts, to size the outputs).

    cc = components(mesh)                              # a label per vertex and face, cc.stats: one row per piece (csrc/mesh_components.hip)
    mesh, report = clean_mesh(mesh, keep_largest=1)    # drop the floaters
    small = simplify_mesh(mesh, target_faces=50000)    # vertex clustering with quadric representatives (csrc/mesh_simplify.hip)
    write_ply("scene_small.ply", small.mesh)
    smooth = smooth_mesh(mesh, iterations=10, max_move=0.5 * h)     # Taubin smoothing over a device-built adjacency (csrc/mesh_smooth.hip)
    n = vertex_normals(smooth.mesh)                    # area-weighted, deterministic"""
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import ops


class Mesh(NamedTuple):
    vertices: torch.Tensor                  # [V,3] f32
    faces: torch.Tensor                     # [T,3] int32, counter-clockwise seen from the outside
    normals: Optional[torch.Tensor]         # [V,3] f32 unit vectors pointing out of the solid (0 where undefined), or None


def marching_tetrahedra(values, iso, sign=+1, lo=(0.0, 0.0, 0.0), h=(1.0, 1.0, 1.0), normals=True):
    """values: device f32 [Nx, Ny, Nz] sampled at lo + (i, j, k) * h; inside is sign * value > sign * iso (+1: a density, -1: a signed
    distance).  normals=True adds the normalised central-difference gradient of the grid, pointing outwards.  An empty surface returns
    empty tensors without an emit launch."""
    workspace, counts = ops.mesh_count(values, iso, sign)
    n_vertices, n_faces = counts.tolist()                               # the one synchronisation: the outputs' sizes
    v, n, f = ops.mesh_emit(values, iso, sign, lo, h, workspace, n_vertices, n_faces, normals=bool(normals))     # checks lo and h
    return Mesh(v, f, n)


def _resolution3(resolution):
    r = (resolution,) * 3 if np.isscalar(resolution) else tuple(resolution)
    if len(r) != 3 or any(int(x) != x or x < 1 for x in r):
        raise ValueError("resolution must be a positive integer or three of them (cells per axis), got %r" % (resolution,))
    return tuple(int(x) for x in r)


def grid_spacing(lo, hi, resolution):
    """(lo, h) as python floats: `resolution` cells per axis between lo and hi, so resolution + 1 points."""
    r = _resolution3(resolution)
    lo, hi = [float(x) for x in lo], [float(x) for x in hi]
    if len(lo) != 3 or len(hi) != 3 or not all(b > a for a, b in zip(lo, hi)):
        raise ValueError("bounds must be lo[3] < hi[3], got %r, %r" % (lo, hi))
    return lo, [(b - a) / n for a, b, n in zip(lo, hi, r)]


def grid_points(lo, h, shape, start, stop, device):
    """Positions [stop - start, 3] (f32) of the grid points with linear indices start .. stop - 1, z fastest: lo + (i, j, k) * h, the
    product and the sum each rounded to f32 -- what sample_grid evaluates and what the extraction places the vertices between."""
    _, ny, nz = shape
    idx = torch.arange(start, stop, device=device, dtype=torch.int64)
    ijk = torch.stack([idx // (ny * nz), idx // nz % ny, idx % nz], 1).to(torch.float32)
    lo_t = torch.tensor(lo, device=device, dtype=torch.float32)
    h_t = torch.tensor(h, device=device, dtype=torch.float32)
    return lo_t + ijk * h_t


def sample_grid(fn, lo, hi, resolution, chunk=2**21, device="cuda"):
    """fn(points [n,3]) -> [n] evaluated on the (resolution + 1)^3 points between lo and hi, `chunk` points per call (it need not
    divide the point count), under torch.no_grad() and in the caller's autocast state -> f32 [Rx+1, Ry+1, Rz+1] on `device`."""
    lo, h = grid_spacing(lo, hi, resolution)
    shape = tuple(n + 1 for n in _resolution3(resolution))
    total = shape[0] * shape[1] * shape[2]
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError("chunk must be positive")
    values = torch.empty(total, device=device, dtype=torch.float32)
    with torch.no_grad():
        for start in range(0, total, chunk):
            stop = min(start + chunk, total)
            out = fn(grid_points(lo, h, shape, start, stop, device))
            if out.numel() != stop - start:
                raise ValueError("fn must return one value per point, got %s for %d points" % (tuple(out.shape), stop - start))
            values[start:stop] = out.reshape(-1).to(torch.float32)
    return values.view(shape)


def extract_mesh(model, resolution, threshold, bounds=None, normals="grid", return_grid=False, sign=+1, chunk=2**21, device=None):
    """The surface density == threshold of `model` (NGP with any encoder, VoxelGrid: model.density, solid where the density is higher),
    or the surface value == threshold of a plain callable points [n,3] -> [n] (sign=-1 for a signed distance; bounds are then required).
    bounds: (lo[3], hi[3]), default the model's [xyz_min, xyz_max]; resolution: cells per axis.
    normals: "grid" -- central differences of the sampled grid; "analytic" -- model.density_normals at the vertices (hash-grid NGP only:
    the other models raise its NotImplementedError); None -- no normals.  return_grid=True also returns the sampled values."""
    if normals not in ("grid", "analytic", None):
        raise ValueError('normals must be "grid", "analytic" or None, got %r' % (normals,))
    is_model = hasattr(model, "density")
    fn = model.density if is_model else model
    if normals == "analytic" and not hasattr(model, "density_normals"):
        raise ValueError('normals="analytic" needs a model with density_normals')
    if bounds is None:
        if not (is_model and hasattr(model, "xyz_min") and hasattr(model, "xyz_max")):
            raise ValueError("bounds=(lo, hi) is required for a plain callable")
        bounds = (model.xyz_min.reshape(3).tolist(), model.xyz_max.reshape(3).tolist())
    if device is None:
        device = model.xyz_min.device if is_model and hasattr(model, "xyz_min") else "cuda"
    lo, h = grid_spacing(bounds[0], bounds[1], resolution)
    values = sample_grid(fn, bounds[0], bounds[1], resolution, chunk=chunk, device=device)
    mesh = marching_tetrahedra(values, threshold, sign=sign, lo=lo, h=h, normals=normals == "grid")
    if normals == "analytic":
        n = model.density_normals(mesh.vertices)[1] if mesh.vertices.shape[0] else mesh.vertices.clone()
        mesh = Mesh(mesh.vertices, mesh.faces, n)
    return (mesh, values) if return_grid else mesh


def topology(mesh):
    """Host-side invariants of a mesh: dict(vertices, faces, euler = V - E + T, boundary_edges = edges used by one face only).  A closed
    surface has no boundary edges; a sphere has euler 2, a torus 0."""
    f = torch.as_tensor(mesh.faces).detach().cpu().numpy().astype(np.int64).reshape(-1, 3)
    n_vertices = int(torch.as_tensor(mesh.vertices).shape[0])
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1)
    _, uses = np.unique(e[:, 0] * max(n_vertices, 1) + e[:, 1], return_counts=True)
    return {"vertices": n_vertices, "faces": int(len(f)), "euler": n_vertices - int(len(uses)) + int(len(f)),
            "boundary_edges": int((uses == 1).sum())}


# ---- the pieces of a mesh (csrc/mesh_components.hip; contract: DESIGN.md section 3, "Connected components") --------------------------
class ComponentStats(NamedTuple):
    """One row per component, on the device."""
    vertices: torch.Tensor                  # [C] int32
    faces: torch.Tensor                     # [C] int32
    edges: torch.Tensor                     # [C] int32: distinct undirected edges of good faces with three distinct indices
    boundary_edges: torch.Tensor            # [C] int32: edges used by exactly one face
    nonmanifold_edges: torch.Tensor         # [C] int32: edges used by three or more faces
    euler: torch.Tensor                     # [C] int32: vertices - edges + faces
    area: torch.Tensor                      # [C] f64: sum of 0.5 |(b - a) x (c - a)|
    volume: torch.Tensor                    # [C] f64: sum of a . (b x c) / 6, signed; the enclosed volume of a closed, outward-oriented piece
    lo: torch.Tensor                        # [C,3] f32: the bounding box
    hi: torch.Tensor                        # [C,3] f32


class MeshComponents:
    """What components() returns.  vertex_component int32 [V] and face_component int32 [T] hold the component number (0 .. n - 1, by
    increasing smallest vertex index) or -1 (an unused vertex, a bad face); n, bad_faces, unused_vertices and rounds are python ints.
    .stats is the ComponentStats table, computed on first use."""

    def __init__(self, vertices, faces, vertex_component, face_component, n, bad_faces, unused_vertices, rounds):
        self.vertices, self.faces = vertices, faces
        self.vertex_component, self.face_component = vertex_component, face_component
        self.n, self.bad_faces, self.unused_vertices, self.rounds = n, bad_faces, unused_vertices, rounds
        self._stats = None

    @property
    def stats(self):
        if self._stats is None:
            table = ops.mesh_components_table(self.faces, self.vertices.shape[0], self.vertex_component, self.face_component, self.n)
            floats = ops.mesh_components_measure(self.vertices, self.faces, self.face_component, table[:, 1].contiguous(), self.bad_faces)
            self._stats = ComponentStats(*[table[:, k].contiguous() for k in range(6)], *floats)
        return self._stats


def components(mesh, strict=True):
    """The connected components of a Mesh or a (vertices, faces) pair of device tensors -> MeshComponents.  Two vertices are connected
    when some face names both (vertex connectivity: two pieces that touch in one vertex are one component; connectivity through shared
    edges only is not offered).  An unwelded file (every face with vertices of its own) falls apart into its faces: weld it first
    (mesh_sdf.weld_vertices).  A face with an index outside [0, V) joins nothing; strict=True raises ValueError when there is one,
    strict=False labels it -1 and counts it."""
    vertices, faces = mesh[0], mesh[1]
    ops._mesh_arrays(vertices)
    vc, fc, counts, rounds = ops.mesh_components_label(faces, vertices.shape[0])
    n, bad, unused = counts.tolist()                                     # the labelling's host read besides the round flags
    if bad and strict:
        raise ValueError("%d of the %d faces name a vertex outside 0..%d (strict=False labels them -1)" % (bad, faces.shape[0], vertices.shape[0] - 1))
    return MeshComponents(vertices, faces, vc, fc, n, bad, unused, rounds)


def select_components(mesh, components, keep):
    """The sub-mesh of the components that keep (bool [C], on either device) marks -> (Mesh, vertex_map int32 [V], face_map int32 [T]).
    Kept vertices and faces stay in their original relative order, faces are re-indexed, normals are carried; the maps hold the new
    index or -1.  Bad faces and unused vertices are always dropped."""
    keep = torch.as_tensor(keep)
    if keep.dtype != torch.bool or tuple(keep.shape) != (components.n,):
        raise ValueError("keep must be bool [%d] (one entry per component), got %s %s" % (components.n, keep.dtype, tuple(keep.shape)))
    v, n, f, vertex_map, face_map = ops.mesh_select(mesh.vertices, mesh.normals, mesh.faces, components.vertex_component,
                                                    components.face_component, keep.to(mesh.faces.device))
    return Mesh(v, f, n), vertex_map, face_map


def component_rule(faces, boundary_edges, area, volume, keep_largest=None, min_faces=0, min_area_fraction=0.0, closed_only=False, by="area"):
    """The rule of clean_mesh on host arrays of C rows -> bool [C].  The filters first (faces >= min_faces, area >= min_area_fraction
    of the total area, no boundary edges); then, of what is left, the keep_largest greatest by `by` ("area", "faces", "volume" = |volume|),
    ties to the lower component number."""
    if by not in ("area", "faces", "volume"):
        raise ValueError('by must be "area", "faces" or "volume", got %r' % (by,))
    if keep_largest is not None and (int(keep_largest) != keep_largest or keep_largest < 0):
        raise ValueError("keep_largest must be None or a non-negative integer, got %r" % (keep_largest,))
    faces, area = np.asarray(faces), np.asarray(area, np.float64)
    keep = faces >= min_faces
    if min_area_fraction > 0.0:
        keep &= area >= min_area_fraction * area.sum()
    if closed_only:
        keep &= np.asarray(boundary_edges) == 0
    if keep_largest is not None:
        size = {"area": area, "faces": faces.astype(np.float64), "volume": np.abs(np.asarray(volume, np.float64))}[by]
        ranked = [c for c in np.argsort(-size, kind="stable") if keep[c]][:int(keep_largest)]
        keep = np.zeros(len(faces), bool)
        keep[ranked] = True
    return keep


def clean_mesh(mesh, keep_largest=None, min_faces=0, min_area_fraction=0.0, closed_only=False, by="area"):
    """Drop the floaters of a mesh -> (Mesh, report).  The rule (component_rule) is evaluated on the host from the per-component table:
    C rows, one read.  With all defaults nothing is dropped except bad faces and unused vertices.  report: components, faces and area
    kept and dropped, the bad faces and unused vertices found, and `kept`, the numbers of the kept components."""
    cc = components(mesh, strict=False)
    s = cc.stats
    rows = torch.stack([s.faces.double(), s.boundary_edges.double(), s.area, s.volume], 1).cpu().numpy()        # the one read
    faces, boundary, area, volume = rows[:, 0].astype(np.int64), rows[:, 1].astype(np.int64), rows[:, 2], rows[:, 3]
    keep = component_rule(faces, boundary, area, volume, keep_largest, min_faces, min_area_fraction, closed_only, by)
    out, _, _ = select_components(mesh, cc, torch.from_numpy(keep))
    report = {"components_kept": int(keep.sum()), "components_dropped": int((~keep).sum()),
              "faces_kept": int(faces[keep].sum()), "faces_dropped": int(faces[~keep].sum()),
              "area_kept": float(area[keep].sum()), "area_dropped": float(area[~keep].sum()),
              "bad_faces": cc.bad_faces, "unused_vertices": cc.unused_vertices, "kept": np.flatnonzero(keep).tolist()}
    return out, report


# ---- a smaller mesh (csrc/mesh_simplify.hip; contract: DESIGN.md section 3, "Simplification") ------------------------------------------
SIMPLIFY_MAX_RESOLUTION = ops.MESH_SIMPLIFY_MAX_CELLS - 1      # cubic cells: one below the per-axis limit, so every key stays below INT64_MAX
SIMPLIFY_MAX_PASSES = 32                  # count passes a target_faces search may take


class SimplifiedMesh(NamedTuple):
    mesh: Mesh                              # the output: one vertex per cluster that a surviving face names
    vertex_map: torch.Tensor                # [V] int32: the output vertex an input vertex became, -1 for a bad vertex or a cluster no face names
    face_map: torch.Tensor                  # [T] int32: the output face, -1 for a collapsed or bad face
    lo: tuple                               # the grid: cell q spans lo + [q, q + 1) h, as python floats (f32 values)
    h: tuple
    grid: tuple                             # cells per axis
    n_clusters: int                         # occupied cells
    bad_faces: int                          # faces with an index outside [0, V) or a bad vertex
    bad_vertices: int                       # vertices with a coordinate that is not finite


def simplify_grid(bounds, cell=None, resolution=None):
    """Host arithmetic: the clustering grid over bounds = (lo[3], hi[3]) -> (lo, h, n), lo and h float32 [3], n three ints.  cell: the
    edge length, a scalar or one per axis; resolution: the number of cells along the longest side (cubic cells).  n_k = ceil(extent_k /
    h_k), at least 1: a vertex on the upper face of the box is clamped into the last cell.  An extent of zero gives one cell."""
    if (cell is None) == (resolution is None):
        raise ValueError("give exactly one of cell and resolution")
    lo, hi = np.asarray(bounds[0], np.float32).reshape(-1), np.asarray(bounds[1], np.float32).reshape(-1)
    if lo.shape != (3,) or hi.shape != (3,) or not (np.isfinite(lo).all() and np.isfinite(hi).all() and (hi >= lo).all()):
        raise ValueError("bounds must be finite lo[3] <= hi[3], got %r" % (bounds,))
    extent = hi.astype(np.float64) - lo.astype(np.float64)
    if cell is not None:
        h = np.broadcast_to(np.asarray(cell, np.float32).reshape(-1), (3,)).copy()
        if not (np.isfinite(h).all() and (h > 0).all()):
            raise ValueError("cell must be positive and finite, got %r" % (cell,))
    else:
        if int(resolution) != resolution or not 1 <= resolution <= SIMPLIFY_MAX_RESOLUTION:
            raise ValueError("resolution must be an integer in 1..2^21 - 1, got %r" % (resolution,))
        longest = float(extent.max())
        h = np.full(3, longest / int(resolution) if longest > 0 else 1.0, np.float32)
        if not (h > 0).all():
            h = np.full(3, 1.0, np.float32)
    n = np.maximum(np.ceil(extent / h.astype(np.float64)), 1.0)
    if resolution is not None:
        n = np.minimum(n, float(resolution))           # h is rounded to float32: the longest side has `resolution` cells, not one more
    if (n > SIMPLIFY_MAX_RESOLUTION).any():
        raise ValueError("the grid would have %s cells per axis, 2^21 or more: use a larger cell" % (n.astype(np.int64).tolist(),))
    return lo, h, tuple(int(x) for x in n)


def target_resolution(count, n_target, n_faces, max_resolution=SIMPLIFY_MAX_RESOLUTION, max_passes=SIMPLIFY_MAX_PASSES):
    """The search of simplify_mesh(target_faces=...), host logic over count(resolution) -> surviving faces.  Resolution 1 leaves no
    face.  It doubles the resolution until the count passes n_target (the upper bracket: the smallest such power of two), then bisects
    between that and the power before; every count is one pass, at most max_passes in all.  -> the finest resolution it found with a
    count <= n_target.  The count is not monotone in the resolution, so this is a good grid, not the best one.  n_target >= n_faces
    needs no pass: the finest grid."""
    if int(n_target) != n_target or n_target < 0:
        raise ValueError("target_faces must be a non-negative integer, got %r" % (n_target,))
    if n_target >= n_faces:
        return max_resolution
    lo, hi, passes, r = 1, None, 0, 2
    while r <= max_resolution and passes < max_passes:
        passes += 1
        if count(r) > n_target:
            hi = r
            break
        lo, r = r, 2 * r
    while hi is not None and hi - lo > 1 and passes < max_passes:
        mid = (lo + hi) // 2
        passes += 1
        if count(mid) <= n_target:
            lo = mid
        else:
            hi = mid
    return lo


def simplify_mesh(mesh, cell=None, resolution=None, target_faces=None, bounds=None, regularization=1e-3, normals=True):
    """A smaller mesh by vertex clustering: the vertices of one grid cell become one vertex, placed where the quadric error of the faces
    around the cell is least (corners and creases stay; regularization=inf places it at the cell's mean instead), faces with two corners
    in one cell disappear -> SimplifiedMesh.  mesh: a Mesh or (vertices f32 [V,3], faces int32 [T,3]) on the device; its normals are
    ignored, normals=True gives the output the normalised area vector of every cluster.  Exactly one of cell (edge length, a scalar or
    one per axis), resolution (cells along the longest side of bounds) and target_faces (a search over the resolution with the count
    phase alone, one host read per pass: target_resolution) sets the grid.  bounds = (lo[3], hi[3]): default the box of the finite
    vertices (one more host read); vertices outside are clamped into the boundary cells.  No vertex moves more than one cell edge per
    axis.  Duplicate output faces are not removed.  The result is deterministic: the same input gives the same bytes."""
    if sum(x is not None for x in (cell, resolution, target_faces)) != 1:
        raise ValueError("give exactly one of cell, resolution and target_faces")
    vertices, faces = mesh[0], mesh[1]
    n_faces, n_vertices = ops._mesh_arrays(vertices, faces)
    if not float(regularization) > 0.0:
        raise ValueError("regularization must be positive (inf: the cluster mean), got %r" % (regularization,))
    dev = vertices.device
    if bounds is None:
        finite = torch.isfinite(vertices).all(1, keepdim=True)
        inf = torch.full((1, 3), float("inf"), device=dev)
        box = torch.stack([torch.cat([torch.where(finite, vertices, inf), inf]).amin(0),
                           torch.cat([torch.where(finite, vertices, -inf), -inf]).amax(0)]).tolist()      # a host read: the grid is the host's
        bounds = box if all(np.isfinite(box[0])) else ([0.0] * 3, [0.0] * 3)
    if n_vertices == 0:                                # nothing to cluster: every face is bad
        lo, h, n = simplify_grid(bounds, cell=cell, resolution=1 if target_faces is not None else resolution)
        empty = Mesh(torch.empty(0, 3, device=dev), torch.empty(0, 3, device=dev, dtype=torch.int32), torch.empty(0, 3, device=dev) if normals else None)
        return SimplifiedMesh(empty, torch.empty(0, device=dev, dtype=torch.int32), torch.full((n_faces,), -1, device=dev, dtype=torch.int32),
                              tuple(lo.tolist()), tuple(h.tolist()), n, 0, n_faces, 0)
    if target_faces is not None:
        resolution = target_resolution(lambda r: int(ops.mesh_simplify_count(vertices, faces, *simplify_grid(bounds, resolution=r)).counts[2]),
                                       target_faces, n_faces)
    lo, h, n = simplify_grid(bounds, cell=cell, resolution=resolution)
    st = ops.mesh_simplify_count(vertices, faces, lo, h, n)
    n_clusters, n_v, n_f, bad_vertices, bad_faces = st.counts.tolist()                # the one synchronisation between the phases
    v, nrm, f = ops.mesh_simplify_emit(vertices, faces, st, n_clusters, n_v, n_f, regularization=regularization, normals=bool(normals))
    return SimplifiedMesh(Mesh(v, f, nrm), st.vertex_map, st.face_map, tuple(lo.tolist()), tuple(h.tolist()), n, n_clusters, bad_faces, bad_vertices)


# ---- smoothing (csrc/mesh_smooth.hip; contract: DESIGN.md section 3, "Smoothing") -------------------------------------------------------
SMOOTH_PASS_BAND = 0.1                    # Taubin's k_pb behind mu=None


class MeshAdjacency(NamedTuple):
    """The vertex adjacency as CSR, on the device: the neighbours of vertex v are neighbours[row_start[v] : row_start[v + 1]], distinct
    and ascending.  Built from the good faces (indices inside [0, V), no repeated index) alone."""
    row_start: torch.Tensor                 # [V + 1] int32
    neighbours: torch.Tensor                # [E2] int32: E2 directed edges, two per undirected edge
    multiplicity: torch.Tensor              # [E2] uint8: the good faces that use the edge, in either orientation; saturates at 255
    vertex_flags: torch.Tensor              # [V] uint8: bit 0 boundary, bit 1 non-manifold, bit 2 unused, bit 3 bad (not finite)
    bad_faces: int
    bad_vertices: int
    boundary_vertices: int

    @property
    def degree(self):
        """[V] int32: the number of distinct neighbours (bad ones included)."""
        return self.row_start[1:] - self.row_start[:-1]

    @property
    def boundary(self):
        """[V] bool: some incident edge is used by exactly one face."""
        return (self.vertex_flags & ops.MESH_FLAG_BOUNDARY) != 0


class SmoothedMesh(NamedTuple):
    mesh: Mesh                              # the input's faces tensor, new vertices, normals recomputed (or None)
    adjacency: MeshAdjacency
    bad_faces: int
    bad_vertices: int


def _trim_adjacency(raw):
    row_start, neighbours, multiplicity, flags, counts = raw
    edges, bad_faces, bad_vertices, boundary_vertices = counts.tolist()          # the one host read
    return MeshAdjacency(row_start, neighbours[:edges], multiplicity[:edges], flags, bad_faces, bad_vertices, boundary_vertices)


def adjacency(mesh):
    """The vertex adjacency of a Mesh or a (vertices, faces) pair of device tensors -> MeshAdjacency.  One host read (the number of
    directed edges, to trim the arrays, with the three counters).  It depends on the set of good faces alone: not on their order, not on
    the rotation of their corners."""
    return _trim_adjacency(ops.mesh_adjacency(mesh[0], mesh[1]))


def vertex_normals(mesh_or_vertices, faces=None):
    """Area-weighted vertex normals f32 [V,3] of a Mesh, a (vertices, faces) pair, or vertices with faces=...: the sum of the area
    vectors (b - a) x (c - a) / 2 of the vertex's good faces, in f64 and in a fixed order, normalised; 0 where that sum is 0 or not
    finite (an unused vertex, area vectors that cancel, a face with a vertex that is not finite).  The weighting is by area, not by
    angle as mesh_sdf.pseudonormals: the two agree on a flat neighbourhood and differ elsewhere.  No host read."""
    vertices = mesh_or_vertices if faces is not None else mesh_or_vertices[0]
    faces = faces if faces is not None else mesh_or_vertices[1]
    return ops.mesh_vertex_normals(vertices, faces)


def taubin_mu(lam, pass_band=SMOOTH_PASS_BAND):
    """Taubin's second factor for the pass band k_pb: mu = 1 / (k_pb - 1 / lam), negative and a little larger than lam in magnitude."""
    lam, pass_band = float(lam), float(pass_band)
    if not lam > 0.0 or not 0.0 < pass_band < 1.0 / lam:
        raise ValueError("pass_band must lie in (0, 1 / lam) for a positive lam, got lam=%r pass_band=%r" % (lam, pass_band))
    return 1.0 / (pass_band - 1.0 / lam)


def smooth_mesh(mesh, iterations=10, lam=0.5, mu=-0.53, pass_band=None, boundary="fixed", fixed=None, max_move=None, normals=True,
                adjacency=None):
    """Taubin's lambda | mu smoothing -> SmoothedMesh.  One iteration moves every vertex towards the mean of its neighbours by the factor
    lam, then by the factor mu (negative: it undoes the shrinkage of the first pass).  mu=None, or a pass_band, sets mu = taubin_mu(lam,
    pass_band or 0.1); mu=0.0 is the plain Laplacian, lam passes only.  boundary: "fixed" -- boundary vertices stay; "curve" -- they smooth
    along the boundary only; "free" -- they are vertices like the others (an open mesh then shrinks inwards).  fixed: bool / uint8 [V] on
    the device, vertices that stay (their neighbours still see them).  max_move: a scalar or three values in world units, the bound on
    every coordinate's displacement from the INPUT position, for any number of iterations (None: no bound).  normals: True -- the result
    carries vertex_normals of the new positions, whether or not the input had normals; False -- it carries none.  The result's mesh
    shares the input's faces tensor.  iterations=0 returns the input positions bit for bit.  Vertices that are not finite stay as they
    are and are left out of their neighbours' means; faces with an index outside [0, V) or a repeated index are ignored; both are counted.
    adjacency: the MeshAdjacency of this mesh's faces if it is at hand; then nothing is read back from the device, otherwise one read
    after the last launch (the counters of the adjacency built here).  Deterministic: the same input gives the same bytes."""
    vertices, faces = mesh[0], mesh[1]
    if mu is None or pass_band is not None:
        mu = taubin_mu(lam, SMOOTH_PASS_BAND if pass_band is None else pass_band)
    raw = None
    if adjacency is None:
        raw = ops.mesh_adjacency(vertices, faces)
        row_start, neighbours, multiplicity, flags = raw[:4]
    else:
        row_start, neighbours, multiplicity, flags = adjacency[:4]
    if max_move is not None:
        max_move = np.broadcast_to(np.asarray(max_move, np.float64).reshape(-1), (3,))
    x = ops.mesh_smooth(vertices, row_start, neighbours, multiplicity, flags, iterations, lam, mu, boundary, fixed, max_move)
    nrm = ops.mesh_vertex_normals(x, faces) if normals else None
    if raw is not None:
        adjacency = _trim_adjacency(raw)
    return SmoothedMesh(Mesh(x, faces, nrm), adjacency, adjacency.bad_faces, adjacency.bad_vertices)


# ---- files (host code) -------------------------------------------------------------------------------------------------------------
def _host(mesh):
    v = np.ascontiguousarray(torch.as_tensor(mesh.vertices).detach().cpu().numpy(), dtype="<f4").reshape(-1, 3)
    f = np.ascontiguousarray(torch.as_tensor(mesh.faces).detach().cpu().numpy(), dtype="<i4").reshape(-1, 3)
    n = None if mesh.normals is None else np.ascontiguousarray(torch.as_tensor(mesh.normals).detach().cpu().numpy(), dtype="<f4").reshape(-1, 3)
    if n is not None and n.shape != v.shape:
        raise ValueError("normals must be [V,3] like the vertices")
    return v, f, n


def _host_colors(colors, n_vertices):
    c = np.ascontiguousarray(torch.as_tensor(colors).detach().cpu().numpy(), dtype="<f4")
    if c.shape != (n_vertices, 3):
        raise ValueError("colors must be [V,3] like the vertices, got %s" % (c.shape,))
    return c


def color_bytes(colors):
    """float colours -> uint8 as the PLY stores them: round(clamp(c, 0, 1) * 255), halves to even; a NaN becomes 0."""
    c = np.nan_to_num(np.asarray(colors, np.float32), nan=0.0)
    return np.rint(np.clip(c, 0.0, 1.0) * np.float32(255.0)).astype(np.uint8)


def write_ply(path, mesh, colors=None):
    """Binary little-endian PLY: float x y z (+ nx ny nz when the mesh has normals) per vertex, uchar 3 + three int32 per face.
    colors [V,3] float: also uchar red green blue per vertex, after the normals, as color_bytes rounds them."""
    v, f, n = _host(mesh)
    props = ["x", "y", "z"] + (["nx", "ny", "nz"] if n is not None else [])
    header = ["ply", "format binary_little_endian 1.0", "element vertex %d" % len(v)] + ["property float %s" % p for p in props] \
        + (["property uchar %s" % p for p in ("red", "green", "blue")] if colors is not None else []) \
        + ["element face %d" % len(f), "property list uchar int vertex_indices", "end_header"]
    rows = np.empty(len(f), dtype=[("n", "u1"), ("idx", "<i4", (3,))])
    rows["n"], rows["idx"] = 3, f
    xyz = (v if n is None else np.concatenate([v, n], 1)).astype("<f4")
    if colors is not None:
        table = np.empty(len(v), dtype=[("f", "<f4", (xyz.shape[1],)), ("c", "u1", (3,))])
        table["f"], table["c"] = xyz, color_bytes(_host_colors(colors, len(v)))
        xyz = table
    with open(path, "wb") as fh:
        fh.write(("\n".join(header) + "\n").encode("ascii"))
        fh.write(xyz.tobytes())
        fh.write(rows.tobytes())


def write_obj(path, mesh, colors=None):
    """Wavefront OBJ: v (and vn) lines with nine significant digits (an f32 survives the round trip), 1-based f lines.  colors [V,3]
    float: the v lines read `v x y z r g b`, the colours unclamped and with nine digits too."""
    v, f, n = _host(mesh)
    with open(path, "w") as fh:
        fh.write("# %d vertices, %d faces\n" % (len(v), len(f)))
        if colors is not None:
            fh.writelines("v %.9g %.9g %.9g %.9g %.9g %.9g\n" % tuple(r) for r in np.concatenate([v, _host_colors(colors, len(v))], 1).tolist())
        else:
            fh.writelines("v %.9g %.9g %.9g\n" % tuple(r) for r in v.tolist())
        if n is not None:
            fh.writelines("vn %.9g %.9g %.9g\n" % tuple(r) for r in n.tolist())
            fh.writelines("f %d//%d %d//%d %d//%d\n" % (a, a, b, b, c, c) for a, b, c in (f + 1).tolist())
        else:
            fh.writelines("f %d %d %d\n" % tuple(r) for r in (f + 1).tolist())


def read_ply(path, return_colors=False):
    """Reads exactly what write_ply writes -> Mesh of CPU tensors, bit for bit.  Any other header (ascii, big endian, other properties
    or elements, polygons that are not triangles) raises ValueError.  return_colors=True: -> (Mesh, colors), colors f32 [V,3] = the
    file's uchar red green blue / 255, or None for a file without them; a file with colours raises without it."""
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.find(b"end_header\n")
    if end < 0:
        raise ValueError("%s: no PLY header" % path)
    lines = data[:end].decode("ascii", "replace").split("\n")[:-1]
    body = data[end + len(b"end_header\n"):]
    xyz, nrm = ["property float %s" % p for p in "xyz"], ["property float %s" % p for p in ("nx", "ny", "nz")]
    rgb = ["property uchar %s" % p for p in ("red", "green", "blue")]
    if len(lines) < 8 or lines[:2] != ["ply", "format binary_little_endian 1.0"] or not lines[2].startswith("element vertex ") \
            or lines[3:6] != xyz or lines[-1] != "property list uchar int vertex_indices" or not lines[-2].startswith("element face ") \
            or lines[6:-2] not in ([[], nrm, rgb, nrm + rgb] if return_colors else [[], nrm]):
        raise ValueError("%s: not the PLY layout write_ply produces (binary little endian, float x y z [nx ny nz], uchar/int faces)" % path)
    try:
        n_v, n_f = int(lines[2].split()[2]), int(lines[-2].split()[2])
    except ValueError:
        raise ValueError("%s: malformed element counts" % path) from None
    coloured = lines[6:-2][-3:] == rgb
    cols = 3 + len(lines[6:-2]) - (3 if coloured else 0)
    stride = 4 * cols + (3 if coloured else 0)
    if n_v < 0 or n_f < 0 or len(body) != stride * n_v + 13 * n_f:
        raise ValueError("%s: the body holds %d bytes, the header announces %d" % (path, len(body), stride * n_v + 13 * n_f))
    table = np.frombuffer(body, np.dtype([("f", "<f4", (cols,))] + ([("c", "u1", (3,))] if coloured else [])), n_v)
    v = table["f"].reshape(n_v, cols)
    rows = np.frombuffer(body, np.dtype([("n", "u1"), ("idx", "<i4", (3,))]), n_f, stride * n_v)
    if n_f and (rows["n"] != 3).any():
        raise ValueError("%s: a face that is not a triangle" % path)
    t = lambda a: torch.from_numpy(np.array(a))                        # a copy: the buffer is read-only
    mesh = Mesh(t(v[:, :3]), t(rows["idx"].astype(np.int32)), t(v[:, 3:]) if cols == 6 else None)
    if not return_colors:
        return mesh
    return mesh, (t(table["c"].reshape(n_v, 3).astype(np.float32) / np.float32(255.0)) if coloured else None)


def read_obj(path, return_colors=False):
    """Reads exactly what write_obj writes -> Mesh of CPU tensors: `v x y z`, then `vn x y z` (as many as vertices) with `f a//a b//b
    c//c`, or no normals with `f a b c`; `#` comments and blank lines are skipped.  Anything else raises ValueError.
    return_colors=True: `v x y z r g b` lines are read too (every v line or none) -> (Mesh, colors f32 [V,3] or None); without it
    such a line raises like any other line write_obj(path, mesh) does not produce."""
    v, n, f, col = [], [], [], []
    with open(path) as fh:
        for no, line in enumerate(fh, 1):
            w = line.split()
            if not w or w[0].startswith("#"):
                continue
            try:
                if return_colors and w[0] == "v" and len(w) == 7:
                    x = [float(s) for s in w[1:]]
                    v.append(x[:3])
                    col.append(x[3:])
                elif w[0] in ("v", "vn") and len(w) == 4:
                    (v if w[0] == "v" else n).append([float(x) for x in w[1:]])
                elif w[0] == "f" and len(w) == 4:
                    idx = []
                    for c in w[1:]:
                        a, sep, b = c.partition("//")
                        if (sep and a != b) or bool(sep) != bool(n):
                            raise ValueError
                        idx.append(int(a))
                    f.append(idx)
                else:
                    raise ValueError
            except ValueError:
                raise ValueError("%s:%d: not what write_obj produces: %r" % (path, no, line.strip())) from None
    if n and len(n) != len(v):
        raise ValueError("%s: %d normals for %d vertices" % (path, len(n), len(v)))
    faces = np.asarray(f, np.int64).reshape(-1, 3) - 1
    if len(faces) and (faces.min() < 0 or faces.max() >= len(v)):
        raise ValueError("%s: a face index outside 1..%d" % (path, len(v)))
    if col and len(col) != len(v):
        raise ValueError("%s: %d coloured vertices of %d" % (path, len(col), len(v)))
    t = lambda a, dt: torch.from_numpy(np.asarray(a, dt).reshape(-1, 3))
    mesh = Mesh(t(v, np.float32), torch.from_numpy(faces.astype(np.int32)), t(n, np.float32) if n else None)
    return (mesh, t(col, np.float32) if col else None) if return_colors else mesh
