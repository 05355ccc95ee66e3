"""The voxel-grid backward kernels' run merge, bit for bit: ngp_voxel_bwd and ngp_voxel_trilinear_bwd against the serial float32
restatement of tests/voxel_runs_reference.py on inputs where no address receives more than two atomic adds, so that the order in which
they arrive cannot show (tests/test_voxel_runs_reference.py holds the conditions).  The tolerance tests of test_gpu_voxel_grid.py and
test_gpu_voxel_trilinear.py cannot see a lane regrouped at a run boundary when the gradients are small; this one can."""
import numpy as np
import pytest
import torch

import voxel_reference as vr
import voxel_runs_reference as ref
from test_voxel_runs_reference import FORMS

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("n", ref.N_SAMPLES)
@pytest.mark.parametrize("trilinear,deg", FORMS)
def test_backward_equals_the_serial_restatement(hip_lib, n, trilinear, deg):
    from ngp_hip import ops
    c = ref.make_case(n, trilinear)
    dsh_ref, dden_ref, n_sh, n_den = ref.merge(deg, c, trilinear)
    assert n_sh.max() <= 2 and n_den.max() <= 2, "an address with three adds: the order of the atomics would show"
    t = {k: torch.from_numpy(v).to(DEV) for k, v in c.items()}
    G, D = ref.G, (deg + 1)**2
    dsh, dden = torch.zeros(G, G, G, 3 * D, device=DEV), torch.zeros(G, G, G, 1, device=DEV)
    ops.voxel_bwd(t["xyzs"], t["dirs"], t["sigmas"], t["rgbs"], t["dsigmas"], t["drgbs"], G, deg, float(vr.grid_min(G, ref.R)),
                  float(ref.R), dsh, dden, trilinear=trilinear)
    dsh, dden = dsh.cpu().numpy().reshape(G**3, 3 * D), dden.cpu().numpy().reshape(G**3)
    print("n=%d trilinear=%s deg=%d: dsh differs at %d of %d touched addresses, ddensity at %d of %d" % (
        n, trilinear, deg, int((dsh.view(np.uint32) != dsh_ref.view(np.uint32)).sum()), int((n_sh > 0).sum()),
        int((dden.view(np.uint32) != dden_ref.view(np.uint32)).sum()), int((n_den > 0).sum())))
    assert np.array_equal(dsh.view(np.uint32), dsh_ref.view(np.uint32))
    assert np.array_equal(dden.view(np.uint32), dden_ref.view(np.uint32))
    untouched = n_sh.sum(1) + n_den == 0
    assert untouched.any() and not dsh[untouched].any() and not dden[untouched].any()
