"""The numpy twin of the pair force field (sclmd_amd/forcefield.py), which defines what the device
kernel must compute, and the C-ABI's host-side checks that need no device."""
import ctypes

import numpy as np
import pytest

import forcefield_cases as FC


@pytest.mark.parametrize("name", sorted(FC.FIELDS))
def test_force_is_minus_energy_gradient(name):
    """force(q) + f0 = -dU/dq by central differences.  h = 1e-5 in mass-weighted units is a
    displacement of 2e-7 A: the truncation error h^2 U'''' / 6 U'' is ~1e-13 relative and the
    rounding error eps U / (h F) ~1e-9, so 1e-6 on the max-norm leaves three orders."""
    ff = FC.FIELDS[name](on_device=False)
    _, q = FC.states(ff, 2)
    h = 1e-5
    for qb in q:
        g = np.empty_like(qb)
        for d in range(len(qb)):
            e = np.zeros_like(qb)
            e[d] = h
            g[d] = (ff.energy(qb + e) - ff.energy(qb - e)) / (2 * h)
        f = ff.absforce(qb)
        assert np.max(np.abs(f + g)) <= 1e-6 * np.max(np.abs(f))
        assert np.array_equal(ff.force(qb), ff.absforce(qb) - ff.f0)


@pytest.mark.parametrize("name", sorted(FC.FIELDS))
def test_pair_forces_sum_to_zero(name):
    ff = FC.FIELDS[name](on_device=False)
    _, q = FC.states(ff, 3)
    F = (ff.absforce(q) / ff.conv).reshape(3, -1, 3)  # Cartesian forces per atom
    assert np.max(np.abs(F.sum(axis=1))) <= 1e-13 * np.max(np.abs(F))


@pytest.mark.parametrize("name", sorted(FC.FIELDS))
def test_dynmat_is_the_linear_part_and_the_states_are_anharmonic(name):
    ff = FC.FIELDS[name](on_device=False)
    D = ff.dynmat()
    assert np.max(np.abs(D - D.T)) <= 1e-14 * np.max(np.abs(D))
    rng = np.random.default_rng(0)
    q = rng.normal(size=D.shape[0]) * 1e-4  # ~2e-6 A: the quadratic term is ~1e-5 of the linear one
    assert np.max(np.abs(ff.force(q) + D @ q)) <= 1e-4 * np.max(np.abs(D @ q))
    _, qs = FC.states(ff, 3)
    assert FC.anharmonic_share(ff, qs) >= 0.01
    # w_max dt < 0.2 at the golden fixtures' time step
    assert np.sqrt(np.max(np.linalg.eigvalsh(D))) * 0.38 < 0.2


def test_batched_force_equals_per_trajectory_calls_and_counts():
    ff = FC.mixed_field(on_device=False)
    _, q = FC.states(ff, 4)
    n0 = ff.ncalls
    fb = ff.force(q)
    assert ff.ncalls == n0 + 4
    for b in range(4):
        assert np.array_equal(fb[b], ff.force(q[b]))
    assert ff.ncalls == n0 + 8


def test_from_cutoff_open_chain():
    ff = FC.morse_field(on_device=False)
    got = sorted(zip(ff.pair_i.tolist(), ff.pair_j.tolist()))
    assert got == sorted([(i, i + 1) for i in range(5)] + [(i, i + 2) for i in range(4)])
    assert ff.shift is None


def test_from_cutoff_periodic_cell_pairs_and_shifts():
    """Two atoms in a cell of length 3 along x, rc = 1.6: the bond inside the cell, the bond through
    the boundary (atom 1 to the image of atom 0 at +3, stored as (0, 1) with shift -3) and nothing
    else; with rc = 3.1 every atom also meets its own image once."""
    from sclmd_amd.forcefield import PairForceField

    axyz = [["C", 0.0, 0.0, 0.0], ["C", 1.5, 0.0, 0.0]]
    ff = PairForceField.from_cutoff(axyz, 1.6, "harmonic", (1.0, 1.5), cell=(3.0, 10.0, 10.0), on_device=False)
    got = sorted((int(i), int(j), tuple(s)) for i, j, s in zip(ff.pair_i, ff.pair_j, ff.shift))
    assert got == [(0, 1, (-3.0, 0.0, 0.0)), (0, 1, (0.0, 0.0, 0.0))]
    ff = PairForceField.from_cutoff(axyz, 3.1, "harmonic", (1.0, 1.5), cell=(3.0, 10.0, 10.0), on_device=False)
    got = sorted((int(i), int(j), tuple(s)) for i, j, s in zip(ff.pair_i, ff.pair_j, ff.shift))
    assert got == [(0, 0, (3.0, 0.0, 0.0)), (0, 1, (-3.0, 0.0, 0.0)), (0, 1, (0.0, 0.0, 0.0)),
                   (1, 1, (3.0, 0.0, 0.0))]
    # an atom and its own image exert no net force on each other's shared coordinates
    _, q = FC.states(ff, 1)
    F = (ff.absforce(q[0]) / ff.conv).reshape(-1, 3)
    assert np.max(np.abs(F.sum(axis=0))) <= 1e-13 * np.max(np.abs(F))


def test_twin_rejects_bad_input():
    from sclmd_amd.forcefield import PairForceField

    a = FC.zigzag()
    with pytest.raises(ValueError, match="out of range"):
        PairForceField(a, [(0, 6)], [0], ["morse"], [(1.0, 1.0, 1.0)])
    with pytest.raises(ValueError, match="zero shift"):
        PairForceField(a, [(2, 2)], [0], ["morse"], [(1.0, 1.0, 1.0)])
    with pytest.raises(ValueError, match="unknown style"):
        PairForceField(a, [(0, 1)], [0], ["buckingham"], [(1.0, 1.0, 1.0)])
    b = [list(x) for x in a]
    b[1][1:] = b[0][1:]
    with pytest.raises(ValueError, match="coincident"):
        PairForceField(b, [(0, 1)], [0], ["morse"], [(1.0, 1.0, 1.0)])


def test_abi_exports_and_null_handle():
    """The three entry points are exported and bound; without a handle they report GLE_ERR_ARG."""
    from sclmd_amd import _native

    lib = _native.load()
    for s in ("gle_set_pair_force", "gle_eval_force", "gle_force_evals"):
        assert s in _native.EXPORTS and s in _native._SIGS and hasattr(lib, s)
    assert lib.gle_eval_force(None, None, None) == -1
    assert lib.gle_force_evals(None, None) == -1
    assert lib.gle_set_pair_force(None, 0, None, None, 0, None, None, None, None, 0, None, None) == -1
    assert (_native.PAIR_HARMONIC, _native.PAIR_MORSE, _native.PAIR_LJ) == (0, 1, 2)
    assert ctypes.sizeof(ctypes.c_int64) == 8
