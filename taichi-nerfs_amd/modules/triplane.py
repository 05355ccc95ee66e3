"""Mirror of reference modules/triplane.py: fp32 tri-plane `TriPlaneEncoder` (:101-204).

The forward gather and the scatter-add backward are the gfx950 kernels ngp_triplane_fwd_f32 / ngp_triplane_bwd_f32.
Three planes (x,y), (y,z), (z,x) of max_res^2 x F floats; every level samples the SAME full-resolution planes (its corners are
mapped to u32(g / res * (max_res - 1))), so several levels write gradient into one entry, and at the top level two neighbouring grid
points can map to one entry (tri-plane encoder).  Output [N, L*F] is feature-major (column j*L + level), as the reference's.
Positions outside [0, 1] are clamped (the reference indexes out of bounds there).
The backward is the TRUE gradient of the forward w.r.t. the table; it depends on the table values.  The reference's glue returns
`params.grad`, which Taichi has already filled, so a leaf parameter gets it twice (2x); Adam is invariant to that factor."""
import torch

from ngp_hip import ops as _ops
from .utils import scale_in_level_np, torch_type


class _TriPlaneEncodeF32(torch.autograd.Function):

    @staticmethod
    def forward(ctx, positions, table, levels):
        ctx.levels = levels
        ctx.save_for_backward(positions, table)
        return _ops.triplane_fwd(positions, table, levels)

    @staticmethod
    def backward(ctx, dout):
        positions, table = ctx.saved_tensors
        dtable = torch.zeros(table.numel(), device=dout.device, dtype=torch.float32)
        _ops.triplane_bwd(positions, dout.contiguous().float(), table, ctx.levels, dtable)
        return None, dtable, None


class TriPlaneEncoder(torch.nn.Module):
    """positions [N,3] f32 in [0,1] -> embedding [N, levels*feature_per_level] f32 (feature-major)."""

    def __init__(self, base_res: int = 16, max_res: int = 2048, levels: int = 16, feature_per_level: int = 2):
        super().__init__()
        if feature_per_level != 4:
            raise ValueError("the tri-plane kernels gather 4 features per entry (NGP builds feature_per_level=4); got %d"
                             % feature_per_level)
        self.base_res = base_res
        self.max_res = max_res
        self.levels = levels
        self.feature_per_level = feature_per_level
        self.out_dim = levels * feature_per_level
        self.log_b = scale_in_level_np(base_res=base_res, max_res=max_res, levels=levels)
        self.total_param_size = int(self.max_res**2) * 3 * self.feature_per_level
        # level table: the in-kernel grid_scale / grid_resolution of the reference (:27-33), done once by the C ABI helper
        self._levels = _ops.make_triplane_levels(base_res, max_res, levels, feature_per_level)
        self.plane_embedding = torch.nn.Parameter(torch.zeros(self.total_param_size, dtype=torch_type), requires_grad=True)
        torch.nn.init.uniform_(self.plane_embedding)      # U(0,1) like reference :148

        print(f'TriPlane Encoder: base_res={base_res} max_res={max_res} levels={levels} feat_per_level={feature_per_level} '
              f'per_level_scale={self.log_b} total_param_size={self.total_param_size} ')

    @property
    def levels_struct(self):
        return self._levels

    def forward(self, positions):
        return _TriPlaneEncodeF32.apply(positions.contiguous(), self.plane_embedding.contiguous(), self._levels)
