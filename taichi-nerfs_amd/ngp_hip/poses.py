"""Camera-pose refinement: a learnable correction per training image, in the parameterisation of ngp_pl's --optimize_ext
(the ancestor of the reference): a rotation dR in axis-angle form applied on the left of R, and a translation dT added to t.

    refiner = PoseRefiner(n_img).cuda()
    batch = batcher.sample(poses=refiner(batcher.poses))        # rays_o / rays_d carry the graph (ngp_sample_rays_bwd)
    loss = ((render(model, batch['rays_o'], batch['rays_d'])['rgb'] - batch['rgb'])**2).mean()
    loss.backward()                                             # -> refiner.dR.grad, refiner.dT.grad (ngp_march_train_bwd on the way)

The 3x3 algebra runs in torch: n_img is tens to hundreds.  The two reductions behind it (samples -> rays, rays -> poses) are the
HIP kernels of csrc/ray_grad.hip."""
import torch
from torch import nn

SMALL_ANGLE_SQ = 1e-2          # theta^2 below which sin(theta)/theta and (1 - cos(theta))/theta^2 are Taylor polynomials in theta^2


class _AddDelta(torch.autograd.Function):
    """x + delta, with x returned bit for bit where delta is zero (x + 0.0 turns a -0.0 of x into +0.0); the gradient is that of the
    sum for both operands everywhere."""

    @staticmethod
    def forward(ctx, x, delta):
        return torch.where(delta == 0, x, x + delta)

    @staticmethod
    def backward(ctx, g):
        return g, g


def _rodrigues_coefficients(theta2):
    """A = sin(theta)/theta and B = (1 - cos(theta))/theta^2 as functions of theta^2, finite with finite derivatives at 0.  Below
    SMALL_ANGLE_SQ: the series to theta^8 (truncation < 3e-14 relative); above: sin(theta)/theta and (sin(theta/2)/(theta/2))^2 / 2,
    which does not cancel like 1 - cos."""
    small = theta2 < SMALL_ANGLE_SQ
    x = torch.where(small, theta2, torch.zeros_like(theta2))
    a_small = 1 + x * (-1 / 6 + x * (1 / 120 + x * (-1 / 5040 + x * (1 / 362880))))
    b_small = 0.5 + x * (-1 / 24 + x * (1 / 720 + x * (-1 / 40320 + x * (1 / 3628800))))
    theta = torch.sqrt(torch.where(small, torch.ones_like(theta2), theta2))        # (the unused branch must not see sqrt'(0))
    half = 0.5 * theta
    a_big = torch.sin(theta) / theta
    b_big = 0.5 * (torch.sin(half) / half)**2
    return torch.where(small, a_small, a_big), torch.where(small, b_small, b_big)


def axis_angle_delta(w):
    """w [n,3] axis-angle -> exp([w]x) - I [n,3,3] by Rodrigues' formula: A K + B K^2 with K the skew matrix of w.  Exactly zero at
    w = 0, with the gradient of the exponential map there (d/dw = the generators)."""
    theta2 = (w * w).sum(-1)
    A, B = _rodrigues_coefficients(theta2)
    zero = torch.zeros_like(w[:, 0])
    K = torch.stack([zero, -w[:, 2], w[:, 1], w[:, 2], zero, -w[:, 0], -w[:, 1], w[:, 0], zero], -1).view(-1, 3, 3)
    return A[:, None, None] * K + B[:, None, None] * (K @ K)


class PoseRefiner(nn.Module):
    """dR [n_img,3] (axis-angle) and dT [n_img,3], zero at the start.  forward(poses [n_img,3,4]) -> [exp(dR) R | t + dT].  At zero
    parameters the input comes back bit for bit, and the gradients with respect to dR, dT are the finite ones of the exponential
    map at the identity."""

    def __init__(self, n_img):
        super().__init__()
        self.dR = nn.Parameter(torch.zeros(int(n_img), 3))
        self.dT = nn.Parameter(torch.zeros(int(n_img), 3))

    def forward(self, poses):
        if poses.ndim != 3 or poses.shape[0] != self.dR.shape[0] or poses.shape[1] < 3 or poses.shape[2] != 4:
            raise ValueError("poses must be [n_img,3,4] with n_img = %d, got %s" % (self.dR.shape[0], tuple(poses.shape)))
        poses = poses[:, :3, :]
        dR, dT = self.dR.to(poses.dtype), self.dT.to(poses.dtype)
        delta = torch.cat([axis_angle_delta(dR) @ poses[:, :, :3], dT[:, :, None]], dim=2)       # (exp(dR) - I) R | dT
        return _AddDelta.apply(poses, delta)
