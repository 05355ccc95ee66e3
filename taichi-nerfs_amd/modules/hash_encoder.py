"""Mirror of reference modules/hash_encoder.py: fp32 multiresolution hash-grid `HashEncoder` (:147-285).

The forward gather and the scatter-add backward are the gfx950 kernels ngp_hash_fwd_f32 / ngp_hash_bwd_f32.
The backward is the TRUE gradient of the forward w.r.t. the table (the reference hands autograd a tensor that
torch then adds to itself, i.e. 2x the gradient -- SURVEY.md H7; Adam is invariant to that factor).

Positions that require grad also receive one (ngp_hash_bwd_input_f32 / _bf16; the reference returns None, :277): the derivative of the
forward as it evaluates -- its f32 cell and fraction, and on a cell face the cell floorf selects.  By default the backwards are ONCE
differentiable.  Positions that do not require grad launch nothing new.

HashEncoder(twice_differentiable=True) selects Functions whose backward is itself an autograd Function (_HashGradF32 / _HashGradBF16):
torch.autograd.grad(..., create_graph=True) then returns a position gradient that carries a graph, and a loss on it (eikonal, normal
smoothness, gradient penalty) trains the table, the layers that produced the incoming gradient and the positions through
ngp_hash_bwd2_gather_* / ngp_hash_bwd2_table_f32 (csrc/hash_grad_input2.hip).  First-order results have the default path's bits.
The table gradient itself is marked non-differentiable: differentiating THROUGH it raises instead of returning something wrong."""
import torch
from torch.autograd.function import once_differentiable

from ngp_hip import ops as _ops
from .utils import scale_in_level_np


class _HashEncodeF32(torch.autograd.Function):

    @staticmethod
    def forward(ctx, positions, table, levels):
        ctx.levels = levels
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(positions, table)              # d enc / d positions reads the table the forward read
        else:
            ctx.save_for_backward(positions)
        ctx.table_numel = table.numel()
        return _ops.hash_fwd_f32(positions, table, levels)

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        positions = ctx.saved_tensors[0]
        dout = dout.contiguous().float()
        dx = dtable = None
        if ctx.needs_input_grad[0]:
            dx = _ops.hash_bwd_input_f32(positions, ctx.saved_tensors[1], dout, ctx.levels)
        if ctx.needs_input_grad[1]:
            dtable = torch.zeros(ctx.table_numel, device=dout.device, dtype=torch.float32)
            _ops.hash_bwd_f32(positions, dout, ctx.levels, dtable)
        return dx, dtable, None


class _HashEncodeBF16(torch.autograd.Function):
    """bf16-stored copy of the fp32 master table in the forward (half the gather bytes), the same fp32 scatter-add
    backward: d(encoding)/d(table) does not depend on the table values."""

    @staticmethod
    def forward(ctx, positions, table, table_bf16, levels):
        ctx.levels = levels
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(positions, table_bf16)         # the copy the forward read, not the fp32 master
        else:
            ctx.save_for_backward(positions)
        ctx.table_numel = table.numel()
        return _ops.hash_fwd_bf16(positions, table_bf16, levels)

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        positions = ctx.saved_tensors[0]
        dout = dout.contiguous().float()
        dx = dtable = None
        if ctx.needs_input_grad[0]:
            dx = _ops.hash_bwd_input_bf16(positions, ctx.saved_tensors[1], dout, ctx.levels)
        if ctx.needs_input_grad[1]:
            dtable = torch.zeros(ctx.table_numel, device=dout.device, dtype=torch.float32)
            _ops.hash_bwd_f32(positions, dout, ctx.levels, dtable)
        return dx, dtable, None, None


class _HashGradF32(torch.autograd.Function):
    """The first backward of the fp32 encoder as a differentiable function of (dout, positions, table): (dx | None, dtable | None) by
    the operators the default path calls.  Its own backward (for ddx = d loss / d dx) is the double backward; dtable is not
    differentiable."""

    @staticmethod
    def forward(ctx, dout, positions, table, levels, need_x, need_table):
        ctx.levels, ctx.dout_dtype = levels, dout.dtype
        ctx.set_materialize_grads(False)
        d = dout.contiguous().float()
        dx = dtable = None
        if need_x:
            dx = _ops.hash_bwd_input_f32(positions, table, d, levels)
            ctx.save_for_backward(d, positions, table)
        if need_table:
            dtable = torch.zeros(table.numel(), device=d.device, dtype=torch.float32)
            _ops.hash_bwd_f32(positions, d, levels, dtable)
            ctx.mark_non_differentiable(dtable)
        return dx, dtable

    @staticmethod
    @once_differentiable
    def backward(ctx, ddx, _ddtable):
        if ddx is None:
            return None, None, None, None, None, None
        d, positions, table = ctx.saved_tensors
        ddx = ddx.contiguous().float()
        need = ctx.needs_input_grad
        d_denc = d_x = d_table = None
        if need[0] or need[1]:
            d_denc, d_x = _ops.hash_bwd2_gather_f32(positions, table, d, ddx, ctx.levels, need_denc=need[0], need_x=need[1])
            if d_denc is not None:
                d_denc = d_denc.to(ctx.dout_dtype)
        if need[2]:
            d_table = torch.zeros(table.numel(), device=d.device, dtype=torch.float32)
            _ops.hash_bwd2_table_f32(positions, d, ddx, ctx.levels, d_table)
            d_table = d_table.view(table.shape)
        return d_denc, d_x, d_table, None, None, None


class _HashGradBF16(torch.autograd.Function):
    """_HashGradF32 for the bf16-copy encoder: dx and its double backward read the bf16 copy the forward read; both table gradients go
    to the fp32 master (neither scatter reads the table)."""

    @staticmethod
    def forward(ctx, dout, positions, table, table_bf16, levels, need_x, need_table):
        ctx.levels, ctx.dout_dtype, ctx.table_shape = levels, dout.dtype, table.shape
        ctx.set_materialize_grads(False)
        d = dout.contiguous().float()
        dx = dtable = None
        if need_x:
            dx = _ops.hash_bwd_input_bf16(positions, table_bf16, d, levels)
            ctx.save_for_backward(d, positions, table_bf16)
        if need_table:
            dtable = torch.zeros(table.numel(), device=d.device, dtype=torch.float32)
            _ops.hash_bwd_f32(positions, d, levels, dtable)
            ctx.mark_non_differentiable(dtable)
        return dx, dtable

    @staticmethod
    @once_differentiable
    def backward(ctx, ddx, _ddtable):
        if ddx is None:
            return None, None, None, None, None, None, None
        d, positions, table_bf16 = ctx.saved_tensors
        ddx = ddx.contiguous().float()
        need = ctx.needs_input_grad
        d_denc = d_x = d_table = None
        if need[0] or need[1]:
            d_denc, d_x = _ops.hash_bwd2_gather_bf16(positions, table_bf16, d, ddx, ctx.levels, need_denc=need[0], need_x=need[1])
            if d_denc is not None:
                d_denc = d_denc.to(ctx.dout_dtype)
        if need[2]:
            d_table = torch.zeros(table_bf16.numel(), device=d.device, dtype=torch.float32)
            _ops.hash_bwd2_table_f32(positions, d, ddx, ctx.levels, d_table)
            d_table = d_table.view(ctx.table_shape)
        return d_denc, d_x, d_table, None, None, None, None


class _HashEncodeF32Twice(torch.autograd.Function):
    """_HashEncodeF32 whose backward is _HashGradF32: differentiable once more."""

    @staticmethod
    def forward(ctx, positions, table, levels):
        ctx.levels = levels
        ctx.save_for_backward(positions, table)
        return _ops.hash_fwd_f32(positions, table, levels)

    @staticmethod
    def backward(ctx, dout):
        positions, table = ctx.saved_tensors
        dx, dtable = _HashGradF32.apply(dout, positions, table, ctx.levels, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return dx, dtable, None


class _HashEncodeBF16Twice(torch.autograd.Function):
    """_HashEncodeBF16 whose backward is _HashGradBF16: differentiable once more."""

    @staticmethod
    def forward(ctx, positions, table, table_bf16, levels):
        ctx.levels = levels
        ctx.save_for_backward(positions, table, table_bf16)
        return _ops.hash_fwd_bf16(positions, table_bf16, levels)

    @staticmethod
    def backward(ctx, dout):
        positions, table, table_bf16 = ctx.saved_tensors
        dx, dtable = _HashGradBF16.apply(dout, positions, table, table_bf16, ctx.levels, ctx.needs_input_grad[0],
                                         ctx.needs_input_grad[1])
        return dx, dtable, None, None


class HashEncoder(torch.nn.Module):
    """positions [N,3] f32 in [0,1] -> embedding [N, levels*feature_per_level] f32 (level-major).

    table_dtype=torch.bfloat16 (not in the reference; BASELINE config 2 names a bf16 hash grid): the forward gathers from
    a bf16 copy of the fp32 master `hash_table` (refreshed whenever the parameter changes, the way hash_encoder_half.py:367
    re-casts its fp16 copy every call); parameter, gradient, optimizer state and state_dict stay fp32.

    twice_differentiable=True: the position gradient can itself be differentiated (autograd.grad(..., create_graph=True) followed
    by a backward of a loss on it); the default keeps the once-differentiable Functions."""

    def __init__(self, max_params: float = 2**19, levels: int = 16, base_res: float = 16.0, max_res: float = 2048.0,
                 feature_per_level: int = 2, table_dtype=None, twice_differentiable: bool = False):
        super().__init__()
        self.twice_differentiable = bool(twice_differentiable)
        if table_dtype not in (None, torch.float32, torch.bfloat16):
            raise ValueError("table_dtype must be None / torch.float32 / torch.bfloat16")
        if table_dtype == torch.bfloat16 and feature_per_level != 2:
            raise ValueError("the bf16 table packs feature pairs: feature_per_level must be 2")
        self.table_dtype = torch.bfloat16 if table_dtype == torch.bfloat16 else torch.float32
        self._bf16, self._bf16_ver = None, None
        levels = int(levels)
        self.log_b = scale_in_level_np(base_res=base_res, max_res=max_res, levels=levels)
        self.base_res = base_res
        self.hash_level = levels
        self.max_params = max_params
        self.feature_per_level = feature_per_level
        self.out_dim = feature_per_level * levels

        # level table: same host arithmetic as reference :183-205, done once by the C ABI helper
        self._levels = _ops.make_levels(max_params, levels, base_res, max_res, feature_per_level)
        _, _, sizes, offsets = _ops.levels_to_numpy(self._levels)
        self.register_buffer('offsets', torch.tensor(offsets.astype('int64'), dtype=torch.int32), persistent=False)
        self.register_buffer('hash_map_sizes', torch.tensor(sizes.astype('int64'), dtype=torch.int32), persistent=False)
        self.begin_fast_hash_level = int(self._levels.begin_fast_hash_level)
        self.total_param_size = int(self._levels.total_entries) * feature_per_level

        print(f'Hash Encoder: base_res={base_res} max_res={max_res} hash_level={levels} '
              f'feat_per_level={feature_per_level} per_level_scale={self.log_b} '
              f'total_hash_size={int(self._levels.total_entries)} ')

        self.hash_table = torch.nn.Parameter(torch.zeros(self.total_param_size, dtype=torch.float32), requires_grad=True)
        torch.nn.init.uniform_(self.hash_table)          # U(0,1) like reference :227

    @property
    def levels_struct(self):
        return self._levels

    def table_bf16(self):
        """The bf16 copy the forward gathers from; re-cast only when the parameter was written through torch (optimizer
        step, load_state_dict -- its version counter moves).  FusedTrainer updates parameter AND copy in its Adam kernel."""
        t = self.hash_table
        ver = (t.data_ptr(), t._version)
        if self._bf16 is None or self._bf16.device != t.device:
            self._bf16, self._bf16_ver = torch.empty(t.shape, device=t.device, dtype=torch.bfloat16), None
        if self._bf16_ver != ver:
            _ops.cast_bf16(t.detach(), self._bf16)
            self._bf16_ver = ver
        return self._bf16

    def forward(self, positions):
        if self.table_dtype == torch.bfloat16:
            fn = _HashEncodeBF16Twice if self.twice_differentiable else _HashEncodeBF16
            return fn.apply(positions.contiguous(), self.hash_table, self.table_bf16(), self._levels)
        fn = _HashEncodeF32Twice if self.twice_differentiable else _HashEncodeF32
        return fn.apply(positions.contiguous(), self.hash_table.contiguous(), self._levels)
