"""The conditions under which tests/voxel_runs_reference.py is an exact statement of the voxel-grid backward (no GPU): the basis is
exact on its directions, no address of any case receives more than two adds, the cases contain what they are there for, and the
restatement's sums are the plain scatter of the same contributions."""
import numpy as np
import pytest

import voxel_reference as vr
import voxel_runs_reference as ref

NEAREST_DEGREES = (0, 2, 4)                # W = 4, 28, 76: many runs per atomic instruction, two, the column loop
TRILINEAR_DEGREES = (0, 1, 2, 3)           # NS = 10, 2, 1 segments per atomic instruction, the column loop
FORMS = [(False, d) for d in NEAREST_DEGREES] + [(True, d) for d in TRILINEAR_DEGREES]


def test_basis_is_exact_along_the_axes():
    """Every basis polynomial is its constant times a small integer there: float32, and float64 rounded to float32, agree to the bit,
    so the order in which a kernel evaluates the polynomial cannot show."""
    d = np.concatenate([ref.AXES, ref.AXES * 2]).astype(np.float64)
    d /= np.sqrt((d * d).sum(1))[:, None]
    a, b = ref.basis(4, d.astype(np.float32)), ref.basis(4, d).astype(np.float32)
    assert a.dtype == np.float32 and a.shape == (12, 25)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert (a != 0).sum() > 12                                             # not only Y_0


@pytest.mark.parametrize("n", ref.N_SAMPLES)
@pytest.mark.parametrize("trilinear", [False, True])
def test_cases_hold_what_they_are_there_for(n, trilinear):
    c = ref.make_case(n, trilinear)
    assert all(v.dtype == np.float32 and len(v) == n for v in c.values())
    u = ref.normalized_index(c["xyzs"])
    lo = -1 if trilinear else 0
    key = np.floor(u) if trilinear else np.rint(u)
    outside = ~((key >= lo) & (key < ref.G)).all(1)
    zero = (c["dsigmas"] == 0) & (c["drgbs"] == 0).all(1)
    assert outside.any() and zero.any() and (c["sigmas"] <= 0).any() and (c["sigmas"] > 0).any()
    assert ((c["rgbs"] > 0) & (c["rgbs"] < 1)).all()
    live = ~outside & ~zero
    flat = (key[:, 0] * 100 + key[:, 1]) * 100 + key[:, 2]
    # every voxel / base cell in one contiguous stretch (inactive samples aside)
    seen = flat[live]
    change = np.flatnonzero(seen[1:] != seen[:-1])
    assert len(np.unique(seen)) == len(change) + 1
    stretch = np.diff(np.concatenate([[0], change + 1, [len(seen)]]))
    assert stretch.min() >= 1 and stretch.max() <= 90
    assert (live[1:] & live[:-1] & (flat[1:] != flat[:-1])).any()          # two runs with no inactive sample between them
    if n > ref.WAVE:                                                       # some stretch continues across a wave boundary
        idx = np.arange(ref.WAVE, n, ref.WAVE)
        assert (live[idx] & live[idx - 1] & (flat[idx] == flat[idx - 1])).any()
    if trilinear:
        cells = np.unique(key[live], axis=0)
        assert (np.abs(cells[:, None] - cells[None]).max(2) + 2 * np.eye(len(cells)) >= 2).all()     # no shared corner row
        assert (cells == -1).any() and (cells == ref.G - 1).any()                                     # corners outside the grid


@pytest.mark.parametrize("n", ref.N_SAMPLES)
@pytest.mark.parametrize("trilinear,deg", FORMS)
def test_no_address_receives_more_than_two_adds(n, trilinear, deg):
    dsh, dden, n_sh, n_den = ref.merge(deg, ref.make_case(n, trilinear), trilinear)
    assert n_sh.max() <= 2 and n_den.max() <= 2
    if n > ref.WAVE:
        assert n_sh.max() == 2 and n_den.max() == 2                        # and the second add is exercised
    assert (n_sh.sum(1) == 0).any() and np.all(dsh[n_sh.sum(1) == 0] == 0) and np.all(dden[n_den == 0] == 0)


@pytest.mark.parametrize("trilinear,deg", FORMS)
def test_restatement_is_the_scatter_of_the_same_contributions(trilinear, deg):
    """Independent of runs and waves: the float64 sum of every live sample's row (times its corner weight) per address."""
    n = ref.N_SAMPLES[-1]
    c = ref.make_case(n, trilinear)
    dsh, dden, _, _ = ref.merge(deg, c, trilinear)
    T, contributes = ref.tile_rows(deg, c)
    T = T.astype(np.float64)
    u = ref.normalized_index(c["xyzs"]).astype(np.float64)
    want, mag = np.zeros((ref.G**3, T.shape[1])), np.zeros((ref.G**3, T.shape[1]))
    for s in np.flatnonzero(contributes):
        if not trilinear:
            corners = [(np.rint(u[s]).astype(int), 1.0)]
        else:
            b = np.floor(u[s]).astype(int)
            f = u[s] - b
            corners = [(b + [i, j, k], (f[0] if i else 1 - f[0]) * (f[1] if j else 1 - f[1]) * (f[2] if k else 1 - f[2]))
                       for i in (0, 1) for j in (0, 1) for k in (0, 1)]
        for q, w in corners:
            if ((q >= 0) & (q < ref.G)).all() and (not trilinear or ((u[s] >= -1) & (u[s] < ref.G)).all()):
                row = (q[0] * ref.G + q[1]) * ref.G + q[2]
                want[row] += w * T[s]
                mag[row] += np.abs(w * T[s])
    got = np.concatenate([dsh, dden[:, None]], 1)
    assert np.all(np.abs(got - want) <= 1e-5 * mag)
    assert np.all(got[mag == 0] == 0) and (mag == 0).any() and (mag > 0).any()
