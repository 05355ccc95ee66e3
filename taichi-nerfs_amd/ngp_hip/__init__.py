"""MI355X-native Instant-NGP hot path: ctypes binding (lib), tensor launchers (ops), SDF surface rendering (surface)."""
from . import lib, ops  # noqa: F401
from . import surface  # noqa: F401
from .ops import resample_rays  # noqa: F401
from .surface import SDFField, SurfaceRenderer, render_surface, surface_render_func  # noqa: F401
