"""Geometry, fields and states shared by the pair-force-field tests (host and GPU).

A 6-atom zigzag that is not collinear in any projection, so all three force components of every atom
are live.  Parameters are carbon-like: the stiffest bond has k = 2 D a^2 = 28 eV/A^2, which with
conv^2 = 0.06466^2 / 12 gives w_max ~ 0.2 and w_max dt < 0.2 at the fixtures' dt = 0.38 (checked in
the tests).  States have max|conv q| = 0.05 A, where a Morse bond with a = 2 / A is ~15 % off its
harmonic force (checked: >= 1 %)."""
import numpy as np

LX = 7.5  # periodic length along the chain for the all-styles case (6 atoms x 1.25 A)
RC = 2.7  # first and second neighbours


def zigzag():
    return [["C", 1.25 * i, 0.35 * (-1) ** i, 0.2 * (i % 3)] for i in range(6)]


def morse_field(on_device=True):
    """Morse on the 5 first- and 4 second-neighbour pairs of the open zigzag (second neighbours are
    stretched far past r0: a nonzero f0)."""
    from sclmd_amd.forcefield import PairForceField

    return PairForceField.from_cutoff(zigzag(), RC, "morse", (3.5, 2.0, 1.45), on_device=on_device)


def mixed_field(on_device=True):
    """All three styles on the zigzag closed into a ring along x through a cell of length LX: Morse on
    the first neighbours inside the cell, Lennard-Jones on those through the boundary (nonzero
    shift), harmonic on the second neighbours."""
    from sclmd_amd.forcefield import HARMONIC, LJ, MORSE, PairForceField

    base = PairForceField.from_cutoff(zigzag(), RC, "harmonic", (1.0, 1.0), cell=(LX, 20.0, 20.0), on_device=False)
    xyz = base.xyz.reshape(-1, 3)
    r = np.linalg.norm(xyz[base.pair_j] + base.shift - xyz[base.pair_i], axis=1)
    crosses = np.any(base.shift != 0.0, axis=1)
    types = np.where(r > 1.8, 1, np.where(crosses, 2, 0))
    assert set(types) == {0, 1, 2} and crosses.any()
    pairs = np.stack([base.pair_i, base.pair_j], axis=1)
    return PairForceField(zigzag(), pairs, types, [MORSE, HARMONIC, LJ],
                          [(3.5, 2.0, 1.45), (2.0, 2.5), (0.3, 1.3)], shift=base.shift, on_device=on_device)


FIELDS = {"morse": morse_field, "mixed": mixed_field}


def states(ff, B, seed=5, amp=0.05):
    """(p, q) of B trajectories, max|conv q| = amp Angstrom per trajectory."""
    rng = np.random.default_rng(seed)
    q = rng.normal(size=(B, len(ff.conv)))
    q *= amp / np.max(np.abs(ff.conv * q), axis=1, keepdims=True)
    p = rng.normal(size=q.shape) * 0.3
    return p, q


def anharmonic_share(ff, q):
    """max-norm distance of the field's force from its harmonic part -dynmat().q, relative."""
    f = ff.force(q)
    fh = -(ff.dynmat() @ np.asarray(q).T).T
    return float(np.max(np.abs(f - fh)) / np.max(np.abs(f)))
