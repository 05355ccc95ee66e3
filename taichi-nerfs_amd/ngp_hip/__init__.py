"""MI355X-native Instant-NGP hot path: ctypes binding (lib), tensor launchers (ops), SDF surface rendering (surface)."""
from . import lib, ops  # noqa: F401
from . import surface  # noqa: F401
from .mesh import read_obj, read_ply  # noqa: F401
from .mesh import ComponentStats, MeshComponents, clean_mesh, components, select_components  # noqa: F401
from .mesh import SimplifiedMesh, simplify_mesh  # noqa: F401
from .mesh import MeshAdjacency, SmoothedMesh, adjacency, smooth_mesh, taubin_mu, vertex_normals  # noqa: F401
from .mesh_sdf import MeshDistance, MeshRayHit, MeshSDF, render_mesh, surface_distance  # noqa: F401
from .mesh import write_obj, write_ply  # noqa: F401
from .mesh_color import VertexColors, bake_field_colors, bake_image_colors  # noqa: F401
from .ops import resample_rays, sdf_eval, sdf_pack, sdf_trace  # noqa: F401
from .surface import SDFField, SurfaceRenderer, render_surface, render_surface_traced, surface_render_func, trace_surface  # noqa: F401
