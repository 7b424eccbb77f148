"""The device-resident pair force field (gle_set_pair_force, sclmd_amd/csrc/gle_force.hip) against
its numpy twin (sclmd_amd.forcefield.PairForceField), which is the definition.

Tolerances: forces 1e-12 relative in max-norm (a few ulps of exp / rsqrt over <= 10 pair terms per
atom with mild cancellation at 5 % strain; the project's fp64 transform tolerance); trajectories,
currents and energies 1e-10 relative, the tolerance test_host_driver_ensemble_per_trajectory_drivers
uses for the same device-vs-host-force comparison.  Geometry, parameters and states: forcefield_cases."""
import ctypes

import numpy as np
import pytest

import forcefield_cases as FC
from conftest import constr_from, load_golden

pytestmark = pytest.mark.gpu

NSTEP = 48


def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def _stepper(ff, B, nmd=8, dt=0.38):
    from sclmd_amd import _native as N

    st = N.Stepper(len(ff.conv), B, nmd, dt)
    st.set_pair_force(ff.xyz, ff.conv, ff.pair_i, ff.pair_j, ff.types, ff.styles, ff.params, ff.shift)
    return st


# ------------------------------------------------------------------------------------ 1. force parity
@pytest.mark.parametrize("B", [1, 3, 40, 65])
@pytest.mark.parametrize("name", sorted(FC.FIELDS))
def test_force_parity(name, B):
    ff = FC.FIELDS[name](on_device=False)
    _, q = FC.states(ff, B)
    assert abs(np.max(np.abs(ff.conv * q)) - 0.05) < 1e-12
    assert FC.anharmonic_share(ff, q) >= 0.01  # a kernel with only the harmonic part right fails below
    want = ff.force(q)
    st = _stepper(ff, B)
    try:
        got = st.eval_force(q)
        assert np.all(st.force_evals() == 0)  # gle_eval_force is not a stepper evaluation
    finally:
        st.close()
    err = rel(got, want)
    print("force parity %s B=%d: %.3e" % (name, B, err))
    assert err <= 1e-12


def test_force_at_rest_is_exactly_zero():
    """force(0) = absforce(0) - f0 is exactly zero on the host; the device takes f0 from its own kernel."""
    ff = FC.morse_field(on_device=False)
    st = _stepper(ff, 3)
    try:
        assert np.all(st.eval_force(np.zeros((3, len(ff.conv)))) == 0.0)
    finally:
        st.close()


# ------------------------------------------------------------------------------ 2. width independence
@pytest.mark.parametrize("name", sorted(FC.FIELDS))
def test_width_independence(name):
    ff = FC.FIELDS[name](on_device=False)
    _, q5 = FC.states(ff, 5)
    st = _stepper(ff, 5)
    try:
        alone = st.eval_force(q5)
    finally:
        st.close()
    _, q64 = FC.states(ff, 64, seed=8)
    st = _stepper(ff, 64)
    try:
        for c in (0, 31, 59):
            q = q64.copy()
            q[c:c + 5] = q5
            assert np.array_equal(st.eval_force(q)[c:c + 5], alone), c
    finally:
        st.close()


# ------------------------------------------------------------------ 3 / 4a. trajectory parity, counts
def _md(case, B, constr, plan, potential, p0, q0, noise=None):
    from sclmd_amd import md as MD
    from sclmd_amd.baths import ebath, phbath

    g = load_golden(case)
    dt, nmd = float(g["dt"]), int(g["nmd"])
    m = MD.md(dt, nmd, float(g["T"]), axyz=FC.zigzag(), dyn=None, ntraj=B, verbose=False, plan_class=plan)
    for i in range(int(g["nbath"])):
        cids = g["b%d_cids" % i]
        if str(g["b%d_kind" % i]) == "ebath":
            b = ebath(cids, 300.0, dt, nmd, bias=float(g["b%d_bias" % i]), efric=g["b%d_efric" % i],
                      exim=g["b%d_exim" % i], zeta1=g["b%d_zeta1" % i], zeta2=g["b%d_zeta2" % i])
        else:
            b = phbath(300.0, cids, 0.2, 10, dt, nmd, ml=int(g["b%d_ml" % i]))
            b.kernel = g["b%d_kernel" % i]
            b.ml = int(g["b%d_ml" % i])
        b.noise = g["b%d_noise" % i] if noise is None else noise[i]
        m.AddBath(b)
    if constr:
        m.AddConstr(constr_from(g))
    m.AddPotential(potential)
    m.p, m.q, m.t = p0.copy(), q0.copy(), 0
    m.ResetHis()
    return m


def _outputs(m):
    return {"p": np.array(m.p), "q": np.array(m.q), "cur": m._st.get_current(), "etot": np.array(m.etot)}


def _run_pair(case, name, B, constr, plan, p0, q0, noise=None, nstep=NSTEP):
    """(device-field outputs, host-field outputs, device evaluation counts, host call counts)."""
    dev = FC.FIELDS[name](on_device=True)
    m = _md(case, B, constr, plan, dev, p0, q0, noise)
    try:
        m.steps(nstep)
        assert m.t == nstep
        od = _outputs(m)
        nd = m._st.force_evals()
    finally:
        m.close()
    hosts = [FC.FIELDS[name](on_device=False) for _ in range(B)]
    n0 = [h.ncalls for h in hosts]
    m = _md(case, B, constr, plan, hosts, p0, q0, noise)
    try:
        for _ in range(nstep):
            m.vv(0)
        oh = _outputs(m)
    finally:
        m.close()
    nh = np.array([h.ncalls - n for h, n in zip(hosts, n0)])
    return od, oh, nd, nh


@pytest.mark.parametrize("plan", ["small", "large"])
@pytest.mark.parametrize("B", [3, 40])
@pytest.mark.parametrize("constr", [False, True])
@pytest.mark.parametrize("case,name", [("vv_mixed", "morse"), ("vv_biased", "mixed")])
def test_trajectory_parity_and_evaluation_counts(case, name, constr, B, plan):
    """md with the device field through steps(48) against md with the same field on the host through
    48 vv calls (a driver call per trajectory at q_t and q~, md.potforce's cache): p, q, every bath's
    current and etot to 1e-10, and as many device evaluations per trajectory as host driver calls
    (n + 1 without constraints: the force at q~ is reused by the next step)."""
    ff = FC.FIELDS[name](on_device=False)
    p0, q0 = FC.states(ff, B, seed=11)
    od, oh, nd, nh = _run_pair(case, name, B, constr, plan, p0, q0)
    for k in ("q", "p", "cur", "etot"):
        err = rel(od[k], oh[k])
        print("%s %s constr=%s B=%d %s: %s %.3e" % (case, name, constr, B, plan, k, err))
        assert err < 1e-10, k
    assert np.array_equal(nd, nh), (nd, nh)
    if not constr:
        assert np.all(nd == NSTEP + 1)


def test_vv_with_device_field_equals_steps():
    """md.vv (gle_step_begin / gle_step_end with fpot == NULL) and md.steps (gle_run) issue the same
    launches with a field set: bitwise equal states."""
    ff = FC.morse_field(on_device=False)
    p0, q0 = FC.states(ff, 3, seed=2)
    out = []
    for use_vv in (False, True):
        m = _md("vv_mixed", 3, True, "auto", FC.morse_field(on_device=True), p0, q0)
        try:
            if use_vv:
                for _ in range(9):
                    m.vv(0)
            else:
                m.steps(9)
            out.append(_outputs(m))
        finally:
            m.close()
    for k in out[0]:
        assert np.array_equal(out[0][k], out[1][k]), k


# ----------------------------------------------------------------------------------- 4b. near hit
@pytest.mark.parametrize("constr", [False, True])
def test_cache_reuse_near_the_evaluated_point(constr):
    """Two trajectories move; the third starts at rest under noise of 1e-16, so every q_t and q~ of it
    lies within 1e-9 of, but not at, the point its force was evaluated at (q = 0, step 0):
    md.potforce reuses that force for the whole run.  The device must do the same -- one evaluation
    -- and follow the host run at 1e-10 on the resting trajectory's own scale (a fresh evaluation
    each step would add -dyn.q, ~1e-2 of the noise force, to it)."""
    B = 3
    g = load_golden("vv_mixed")
    ff = FC.morse_field(on_device=False)
    p0, q0 = FC.states(ff, B, seed=3)
    p0[2] = 0.0
    q0[2] = 0.0
    noise = []
    for i in range(int(g["nbath"])):
        n = np.broadcast_to(g["b%d_noise" % i], (B,) + g["b%d_noise" % i].shape).copy()
        n[2] = 1e-16
        noise.append(n)
    od, oh, nd, nh = _run_pair("vv_mixed", "morse", B, constr, "auto", p0, q0, noise)
    assert np.array_equal(nd, nh), (nd, nh)
    assert nd[2] == 1 and nh[2] == 1
    assert 0.0 < np.max(np.abs(oh["q"][2])) < 1e-9
    for k in ("q", "p"):
        assert rel(od[k][:2], oh[k][:2]) < 1e-10, k
        err = rel(od[k][2], oh[k][2])
        print("resting trajectory constr=%s %s: %.3e" % (constr, k, err))
        assert err < 1e-10, k


@pytest.mark.parametrize("constr", [False, True])
def test_cache_distance_is_measured_from_the_evaluated_point(constr):
    """The third trajectory starts at q = 0 with a momentum of 3e-10 and no noise: each step moves
    it by ~1.1e-10, less than 1e-9, but it leaves the 1e-9 ball around the point of its last
    evaluation every ~9 steps.  md.potforce then evaluates again (and only then).  A cache measured
    against the previous step's q~ instead of the evaluated point would never miss after step 0: the
    counts must equal the host's, which lie strictly between 1 and one per step.

    Tolerance of the drifting trajectory itself: at |q| ~ 5e-9 its force conv F(q) - f0 ~ dyn q ~ 2e-10
    is the difference of two numbers of size |f0|, so the device and the host force, which agree to
    the force tolerance 1e-12 relative to that size (test_force_parity), differ by up to
    dF = 1e-12 |f0|_max in absolute terms whatever the kernel does.  Over n steps that moves p by at
    most dF n dt and q by at most dF (n dt)^2 / 2: these are the bounds (a force taken at a stale
    point is off by ~dyn 1e-9 ~ 4e-11, three orders above dF).  The moving trajectories keep 1e-10."""
    B = 3
    g = load_golden("vv_mixed")
    ff = FC.morse_field(on_device=False)
    p0, q0 = FC.states(ff, B, seed=3)
    p0[2] = 3e-10
    q0[2] = 0.0
    noise = []
    for i in range(int(g["nbath"])):
        n = np.broadcast_to(g["b%d_noise" % i], (B,) + g["b%d_noise" % i].shape).copy()
        n[2] = 0.0
        noise.append(n)
    od, oh, nd, nh = _run_pair("vv_mixed", "morse", B, constr, "auto", p0, q0, noise)
    print("drifting trajectory constr=%s: host calls %s device evaluations %s" % (constr, nh, nd))
    assert 2 < nh[2] < NSTEP // 2  # the host re-evaluates a few times, far from every step
    assert np.max(np.abs(oh["q"][2])) > 2e-9  # ... because it drifted through several 1e-9 balls
    assert np.array_equal(nd, nh), (nd, nh)
    dF = 1e-12 * np.max(np.abs(ff.f0))
    T = NSTEP * float(g["dt"])
    for k, bound in (("q", dF * T * T / 2), ("p", dF * T)):
        assert rel(od[k][:2], oh[k][:2]) < 1e-10, k
        err = float(np.max(np.abs(od[k][2] - oh[k][2])))
        print("drifting trajectory constr=%s %s: abs err %.3e bound %.3e" % (constr, k, err, bound))
        assert err <= bound, k


def test_replacing_the_field_mid_run_starts_from_an_empty_cache():
    """A handle runs with field A, is given field B while live, and goes on: from there it must equal
    a handle that got field B fresh at that state (p, q, t and the baths' histories).  Without
    constraints q_t equals the cached point bitwise at the switch, so a cache that was not emptied for
    every thread of the launch would keep A's force for some or all atoms at the first step (A and B
    differ by tens of percent).  1e-10 as for the trajectories above: the fresh handle rebuilds its
    memory sums from the history, which differs from the running sums at rounding level."""
    from sclmd_amd import _native as N

    g = load_golden("vv_mixed")
    B = 40
    nb = int(g["nbath"])
    ffa = FC.morse_field(on_device=False)
    ffb = FC.mixed_field(on_device=False)
    p0, q0 = FC.states(ffa, B, seed=13)
    assert FC.anharmonic_share(ffb, q0) >= 0.01
    assert rel(ffa.force(q0), ffb.force(q0)) > 0.1

    def stepper():
        st = N.Stepper(len(ffa.conv), B, int(g["nmd"]), float(g["dt"]))
        for i in range(nb):
            kind = N.GLE_BATH_ELECTRON if str(g["b%d_kind" % i]) == "ebath" else N.GLE_BATH_PHONON
            st.add_bath(kind, g["b%d_cids" % i], g["b%d_kernel" % i])
        return st

    def set_field(st, ff):
        st.set_pair_force(ff.xyz, ff.conv, ff.pair_i, ff.pair_j, ff.types, ff.styles, ff.params, ff.shift)

    def noise(st):
        for i in range(nb):
            st.set_noise(i, np.broadcast_to(g["b%d_noise" % i], (B,) + g["b%d_noise" % i].shape))

    live = stepper()
    fresh = stepper()
    try:
        set_field(live, ffa)
        live.set_state(p0, q0, 0)
        for i in range(nb):
            live.set_history(i, None)
        noise(live)
        live.run(5)
        p, q, t = live.get_state()
        hist = [live.get_history(i) for i in range(nb)]
        assert np.all(live.force_evals() == 6)
        set_field(live, ffb)
        live.run(7)
        assert np.all(live.force_evals() == 6 + 8)  # the first step after the switch evaluates at q_t too

        set_field(fresh, ffb)
        fresh.set_state(p, q, t)
        for i in range(nb):
            fresh.set_history(i, hist[i])
        noise(fresh)
        fresh.run(7)
        assert np.all(fresh.force_evals() == 8)
        pl, ql, tl = live.get_state()
        pf, qf, tf = fresh.get_state()
        assert tl == tf == 12
        errs = (rel(ql, qf), rel(pl, pf), rel(live.get_force(), fresh.get_force()))
        print("field replaced mid-run: q %.3e p %.3e f %.3e" % errs)
        assert max(errs) < 1e-10
    finally:
        live.close()
        fresh.close()


# -------------------------------------------------------------------------------------- 5. misuse
def _raw_set(st, ff, **over):
    """gle_set_pair_force through the raw binding with single arguments replaced: (code, message)."""
    a = dict(natom=ff.natom, xyz0=ff.xyz.copy(), conv=ff.conv.copy(), pair_i=ff.pair_i.copy(),
             pair_j=ff.pair_j.copy(), types=ff.types.astype(np.int32), shift=ff.shift,
             styles=ff.styles.astype(np.int32), params=ff.params.copy())
    a.update(over)
    D, I64, I32 = (ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32))
    keep = [np.ascontiguousarray(a["xyz0"], dtype=np.float64), np.ascontiguousarray(a["conv"], dtype=np.float64),
            np.ascontiguousarray(a["pair_i"], dtype=np.int64), np.ascontiguousarray(a["pair_j"], dtype=np.int64),
            np.ascontiguousarray(a["types"], dtype=np.int32),
            None if a["shift"] is None else np.ascontiguousarray(a["shift"], dtype=np.float64),
            np.ascontiguousarray(a["styles"], dtype=np.int32), np.ascontiguousarray(a["params"], dtype=np.float64)]
    rc = st.lib.gle_set_pair_force(
        st.h, int(a["natom"]), keep[0].ctypes.data_as(D), keep[1].ctypes.data_as(D), len(keep[2]),
        keep[2].ctypes.data_as(I64), keep[3].ctypes.data_as(I64), keep[4].ctypes.data_as(I32),
        None if keep[5] is None else keep[5].ctypes.data_as(D), len(keep[6]), keep[6].ctypes.data_as(I32),
        keep[7].ctypes.data_as(D))
    return rc, st.lib.gle_last_error(st.h).decode()


def test_misuse_is_reported_not_run():
    """Every bad field is rejected on the host with GLE_ERR_ARG and a message, nothing is uploaded and
    the field set before stays in force."""
    from sclmd_amd import _native as N

    ff = FC.mixed_field(on_device=False)
    _, q = FC.states(ff, 2)
    st = _stepper(ff, 2)
    try:
        before = st.eval_force(q)

        def with_(arr, idx, val):
            arr = arr.copy()
            arr[idx] = val
            return arr

        same = ff.xyz.copy()
        same[3:6] = same[0:3]  # atoms 0 and 1 (a listed pair) coincide
        bad = {
            "index out of range": dict(pair_j=with_(ff.pair_j, 0, ff.natom)),
            "negative index": dict(pair_i=with_(ff.pair_i, 1, -1)),
            "type out of range": dict(types=with_(ff.types.astype(np.int32), 0, 3)),
            "i == j with zero shift": dict(pair_j=with_(ff.pair_j, 0, ff.pair_i[0]),
                                          shift=with_(ff.shift, 0, 0.0)),
            "unknown style": dict(styles=with_(ff.styles.astype(np.int32), 1, 7)),
            "r0 <= 0": dict(params=with_(ff.params, (0, 2), 0.0)),
            "a <= 0": dict(params=with_(ff.params, (0, 1), -2.0)),
            "sigma not finite": dict(params=with_(ff.params, (2, 1), np.inf)),
            "harmonic r0 NaN": dict(params=with_(ff.params, (1, 1), np.nan)),
            "coincident atoms": dict(xyz0=same),
            "non-finite shift": dict(shift=with_(ff.shift, (0, 0), np.nan)),
        }
        for what, over in bad.items():
            rc, msg = _raw_set(st, ff, **over)
            assert rc == -1 and "pair force" in msg, (what, rc, msg)
            assert np.array_equal(st.eval_force(q), before), what
        rc, msg = _raw_set(st, ff)
        assert rc == 0, msg
    finally:
        st.close()
    # nph != 3 natom
    st = N.Stepper(len(ff.conv) + 3, 2, 8, 0.38)
    try:
        rc, msg = _raw_set(st, ff)
        assert rc == -1 and "natom" in msg
        with pytest.raises(N.GLEError, match="GLE_ERR_STATE"):
            st.eval_force(np.zeros((2, len(ff.conv) + 3)))
    finally:
        st.close()


def _harmonic_stepper(g, B):
    from sclmd_amd import _native as N

    nph = 3 * int(g["natom"])
    st = N.Stepper(nph, B, int(g["nmd"]), float(g["dt"]))
    for i in range(int(g["nbath"])):
        kind = N.GLE_BATH_ELECTRON if str(g["b%d_kind" % i]) == "ebath" else N.GLE_BATH_PHONON
        st.add_bath(kind, g["b%d_cids" % i], g["b%d_kernel" % i])
    return st, nph


def test_no_potential_still_fails_and_removal_restores_the_harmonic_run():
    """Without dyn and without a field gle_run fails as before.  With dyn, a handle that had a field
    (unused, or used for some steps) and lost it (npair = 0) runs the harmonic steps of a handle that
    never had one, bit for bit."""
    from sclmd_amd import _native as N
    from sclmd_amd.forcefield import PairForceField

    g = load_golden("vv_mixed")
    B = 3
    rng = np.random.default_rng(4)
    st, nph = _harmonic_stepper(g, B)
    p0 = g["p0"][None] * (1 + 0.1 * rng.normal(size=(B, 1)))
    q0 = g["q0"][None] * (1 + 0.1 * rng.normal(size=(B, 1)))
    try:
        st.set_state(p0, q0, 0)
        for i in range(int(g["nbath"])):
            st.set_noise(i, np.broadcast_to(g["b%d_noise" % i], (B,) + g["b%d_noise" % i].shape))
        with pytest.raises(N.GLEError, match="no potential force"):
            st.run(1)
    finally:
        st.close()

    axyz = [["C", 1.4 * i, 0.3 * (i % 2), 0.0] for i in range(int(g["natom"]))]
    ff = PairForceField.from_cutoff(axyz, 1.6, "morse", (3.5, 2.0, 1.45), on_device=False)

    def run(mode):
        st, _ = _harmonic_stepper(g, B)
        try:
            st.set_dyn(g["dyn_md"])
            if mode != "never":
                st.set_pair_force(ff.xyz, ff.conv, ff.pair_i, ff.pair_j, ff.types, ff.styles, ff.params, ff.shift)
            if mode == "unused":
                st.clear_pair_force()
            st.set_state(p0, q0, 0)
            for i in range(int(g["nbath"])):
                st.set_history(i, None)
                st.set_noise(i, np.broadcast_to(g["b%d_noise" % i], (B,) + g["b%d_noise" % i].shape))
            if mode == "used":
                st.run(5)
                assert np.all(st.force_evals() == 6)
                st.clear_pair_force()
                st.set_state(p0, q0, 0)
                for i in range(int(g["nbath"])):
                    st.set_history(i, None)
            st.run(20)
            p, q, t = st.get_state()
            assert t == 20
            return p, q, st.get_current(), st.get_energy()
        finally:
            st.close()

    ref = run("never")
    for mode in ("unused", "used"):
        got = run(mode)
        for a, b in zip(got, ref):
            assert np.array_equal(a, b), mode
