"""Anharmonic pair force field with the plugin surface of the host drivers (drivers.py: .force(q),
.absforce, .initforce(), .f0, .axyz, .conv, .quit(), .dynmat()) that can also live on the device.

The field is a fixed list of atom pairs.  Each pair has a type, each type a style and up to four
parameters (eV, Angstrom):

    HARMONIC (0)  U = k/2 (r - r0)^2                      params (k, r0)
    MORSE    (1)  U = D (1 - exp(-a (r - r0)))^2           params (D, a, r0)
    LJ       (2)  U = 4 eps ((sigma/r)^12 - (sigma/r)^6)   params (eps, sigma)

with r = |x_j + shift_ij - x_i| and x = xyz + conv * q, conv = md2ang / sqrt(mass) per DOF, exactly
the coordinates lammpsdriver.force builds (lammpsdriver.py:70-84).  force(q) = conv * F(q) - f0 with
f0 = conv * F(0).  `shift` is an optional per-pair image vector, so a periodic cell can be written as
a static list.

Limits: the list is static -- no cutoff test at run time, no list rebuild -- which suits a junction
whose atoms do not diffuse past each other; a pair keeps interacting however far it stretches and a
pair that is not listed never interacts.  No on-site term, no many-body styles.

The numpy code here is the definition; with on_device=True md.AddPotential uploads the same field
through gle_set_pair_force and md.steps / md.Run stay on the device (sclmd_amd/csrc/gle_force.hip).
"""
import numpy as np

from . import units as U

HARMONIC, MORSE, LJ = 0, 1, 2
STYLES = {"harmonic": HARMONIC, "morse": MORSE, "lj": LJ}
_NPAR = {HARMONIC: 2, MORSE: 3, LJ: 2}


def _style_id(s):
    if isinstance(s, str):
        if s.lower() not in STYLES:
            raise ValueError("PairForceField: unknown style %r" % (s,))
        return STYLES[s.lower()]
    s = int(s)
    if s not in _NPAR:
        raise ValueError("PairForceField: unknown style %d" % s)
    return s


class PairForceField:
    def __init__(self, axyz, pairs, types, styles, params, shift=None, md2ang=0.06466, on_device=True):
        self.axyz = [list(a) for a in axyz]
        self.md2ang = md2ang
        self.on_device = bool(on_device)
        masses = [U.AtomicMassTable[a[0]] for a in self.axyz]
        self.conv = md2ang * np.array([3 * [1.0 / np.sqrt(m)] for m in masses]).flatten()
        self.xyz = np.array([a[1:] for a in self.axyz], dtype=float).flatten()
        self.natom = len(self.axyz)
        pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
        self.pair_i, self.pair_j = pairs[:, 0].copy(), pairs[:, 1].copy()
        self.npair = len(pairs)
        if self.npair == 0:
            raise ValueError("PairForceField: empty pair list")
        self.types = np.broadcast_to(np.asarray(types, dtype=np.int64), (self.npair,)).copy()
        if np.ndim(styles) == 0:
            styles = [styles]
        self.styles = np.array([_style_id(s) for s in styles], dtype=np.int32)
        if not isinstance(params[0], (list, tuple, np.ndarray)):  # one type given as a flat row
            params = [params]
        par = [[float(v) for v in p] for p in params]
        if len(par) != len(self.styles):
            raise ValueError("PairForceField: %d styles but %d parameter rows" % (len(self.styles), len(par)))
        self.params = np.zeros((len(self.styles), 4))
        for k, p in enumerate(par):
            n = _NPAR[int(self.styles[k])]
            if len(p) < n:
                raise ValueError("PairForceField: type %d needs %d parameters" % (k, n))
            self.params[k, :n] = p[:n]
        if self.pair_i.min() < 0 or self.pair_j.min() < 0 or max(self.pair_i.max(), self.pair_j.max()) >= self.natom:
            raise ValueError("PairForceField: atom index out of range")
        if self.types.min() < 0 or self.types.max() >= len(self.styles):
            raise ValueError("PairForceField: pair type out of range")
        self.shift = None if shift is None else np.asarray(shift, dtype=float).reshape(self.npair, 3).copy()
        self._sh = np.zeros((self.npair, 3)) if self.shift is None else self.shift
        if np.any((self.pair_i == self.pair_j) & np.all(self._sh == 0.0, axis=1)):
            raise ValueError("PairForceField: i == j with zero shift")
        self._st = self.styles[self.types]
        self._p = self.params[self.types]
        self.ncalls = 0
        self.initforce()

    # ---------------------------------------------------------------------------- pair terms
    def _geom(self, q):
        q = np.asarray(q, dtype=float)
        x = (self.xyz + self.conv * q).reshape(q.shape[:-1] + (self.natom, 3))
        d = x[..., self.pair_j, :] + self._sh - x[..., self.pair_i, :]
        return d, np.sqrt(np.sum(d * d, axis=-1))

    def _du(self, r):
        """(U, U', U'') of every pair at distances r (..., npair)."""
        p, st = self._p, self._st
        u, du, ddu = np.zeros_like(r), np.zeros_like(r), np.zeros_like(r)
        m = st == HARMONIC
        if m.any():
            k, r0, x = p[m, 0], p[m, 1], r[..., m]
            u[..., m], du[..., m], ddu[..., m] = 0.5 * k * (x - r0) ** 2, k * (x - r0), k + 0.0 * x
        m = st == MORSE
        if m.any():
            D, a, r0, x = p[m, 0], p[m, 1], p[m, 2], r[..., m]
            e = np.exp(-a * (x - r0))
            u[..., m] = D * (1.0 - e) ** 2
            du[..., m] = 2.0 * D * a * e * (1.0 - e)
            ddu[..., m] = 2.0 * D * a * a * e * (2.0 * e - 1.0)
        m = st == LJ
        if m.any():
            eps, sg, x = p[m, 0], p[m, 1], r[..., m]
            s6 = (sg / x) ** 6
            u[..., m] = 4.0 * eps * (s6 * s6 - s6)
            du[..., m] = -24.0 * eps * (2.0 * s6 * s6 - s6) / x
            ddu[..., m] = 4.0 * eps * (156.0 * s6 * s6 - 42.0 * s6) / (x * x)
        return u, du, ddu

    def energy(self, q):
        """Potential energy (eV) at the mass-weighted displacement q (..., nph)."""
        _, r = self._geom(q)
        return np.sum(self._du(r)[0], axis=-1)

    def absforce(self, q):
        """conv * F(q), F the Cartesian force (eV / Angstrom) of the listed pairs; q (nph,) or (..., nph)."""
        q = np.asarray(q, dtype=float)
        self.ncalls += int(np.prod(q.shape[:-1])) if q.ndim > 1 else 1
        d, r = self._geom(q)
        fp = (self._du(r)[1] / r)[..., None] * d          # force on atom i of each pair
        F = np.zeros(q.shape[:-1] + (self.natom, 3)).reshape(-1, self.natom, 3)
        fp = fp.reshape(-1, self.npair, 3)
        np.add.at(F, (slice(None), self.pair_i), fp)
        np.subtract.at(F, (slice(None), self.pair_j), fp)
        return self.conv * F.reshape(q.shape)

    def initforce(self):
        d, r = self._geom(np.zeros(3 * self.natom))
        if not np.all(r > 0.0):
            raise ValueError("PairForceField: coincident atoms in a pair at q = 0")
        self.f0 = self.absforce(np.zeros(3 * self.natom))

    def force(self, q):
        return self.absforce(q) - self.f0

    def dynmat(self, q=None):
        """Analytic mass-weighted Hessian at q = 0: force(q) = -dynmat() q + O(q^2)."""
        d, r = self._geom(np.zeros(3 * self.natom))
        _, du, ddu = self._du(r)
        n = d / r[:, None]
        nn = n[:, :, None] * n[:, None, :]
        K = ddu[:, None, None] * nn + (du / r)[:, None, None] * (np.eye(3) - nn)
        H = np.zeros((self.natom, 3, self.natom, 3))
        for k in range(self.npair):
            i, j = self.pair_i[k], self.pair_j[k]
            H[i, :, i, :] += K[k]
            H[j, :, j, :] += K[k]
            H[i, :, j, :] -= K[k]
            H[j, :, i, :] -= K[k]
        H = H.reshape(3 * self.natom, 3 * self.natom)
        return self.conv[:, None] * H * self.conv[None, :]

    def quit(self):
        pass

    # ---------------------------------------------------------------------------- construction
    @classmethod
    def from_cutoff(cls, axyz, rc, style, params, cell=None, **kw):
        """One pair type between every two atoms closer than rc in the reference geometry.  cell:
        None, three box lengths or a (3, 3) matrix of cell vectors (rows); with a cell the pairs
        through the nearest images get their image vector as `shift` (requires rc <= half the
        shortest cell height for the list to be complete, as any minimum-image list)."""
        xyz = np.array([a[1:] for a in axyz], dtype=float)
        na = len(xyz)
        images = [np.zeros(3)]
        if cell is not None:
            c = np.asarray(cell, dtype=float)
            c = np.diag(c) if c.ndim == 1 else c
            images = [i * c[0] + j * c[1] + k * c[2] for i in (0, 1, -1) for j in (0, 1, -1) for k in (0, 1, -1)]
        pairs, shifts = [], []
        for i in range(na):
            for j in range(i, na):
                for m, s in enumerate(images):
                    if i == j and (m == 0 or any(np.allclose(s, -t) for t in images[1:m])):
                        continue  # an atom and its own image: each +-s once
                    if np.linalg.norm(xyz[j] + s - xyz[i]) < rc:
                        pairs.append((i, j))
                        shifts.append(s)
        if not pairs:
            raise ValueError("PairForceField.from_cutoff: no pair within rc = %g" % rc)
        shift = np.array(shifts) if cell is not None else None
        return cls(axyz, pairs, np.zeros(len(pairs), dtype=np.int64), [style], [params], shift=shift, **kw)
