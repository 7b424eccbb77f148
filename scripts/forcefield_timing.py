#!/usr/bin/env python3
"""Step cost of the device-resident pair force field at a C3-sized junction (synthetic.junction("C3")
geometry and baths, Morse bonds between nearest neighbours, 64 trajectories), microseconds per step
over --steps steps after a warm-up:

  device    the field on the device through md.steps(n) (gle_run: no host round trip per step)
  host      the same field with on_device=False: a q~ download, a Python force call per trajectory
            and an Fc upload twice per step (the only way to run this potential without the field)
  harmonic  dyn = ff.dynmat() on the two-launch path (gle_step_begin / gle_step_end, no host force)

device - harmonic is the field's cost on the step's critical path; host / device its gain.  Each
variant runs in a child process of its own under a time limit; the first failure ends the script.
Prints one JSON line per variant and a summary line.  The force kernels' own durations come from a
kernel trace of `--variant device` (see profiles/forcefield/README.md)."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VARIANTS = ("device", "host", "harmonic")


def field(axyz, on_device):
    from sclmd_amd.forcefield import PairForceField

    return PairForceField.from_cutoff(axyz, 1.5, "morse", (3.5, 2.0, 1.42), on_device=on_device)


def run_variant(args):
    from sclmd_amd import md as MD
    from sclmd_amd import synthetic

    B = args.ntraj
    _, axyz, baths, meta = synthetic.junction("C3", seed=1234, ml=args.ml, nmd=args.nmd, gmem_device=True)
    ff = field(axyz, args.variant == "device")
    m = MD.md(meta["dt"], meta["nmd"], meta["T"], axyz=axyz, dyn=ff.dynmat() if args.variant == "harmonic" else None,
              ntraj=B, verbose=False)
    for b in baths:
        m.AddBath(b)
    if args.variant != "harmonic":
        m.AddPotential(ff)
    rng = np.random.default_rng(7)
    for b in baths:
        b.noise = rng.standard_normal((B, meta["nmd"], b.nc)) * 1e-3
    m.p = rng.normal(size=(B, meta["nph"])) * 1e-3
    m.q = rng.normal(size=(B, meta["nph"])) * 1e-3
    m.t = 0
    m.ResetHis()
    st = m._ensure_device()
    m.steps(0)  # uploads the noise

    def advance(n):
        if args.variant == "harmonic":  # the two-launch path (gle_run would take the composed step)
            for _ in range(n):
                st.step_begin(None, want_qt=False)
                st.step_end(None)
            m._dev_newer = True
        else:
            m.steps(n)

    advance(args.warmup)
    st.sync()
    ev0 = st.force_evals().sum()
    t0 = time.perf_counter()
    advance(args.steps)
    st.sync()
    wall = time.perf_counter() - t0
    npair = ff.npair
    out = {"variant": args.variant, "ntraj": B, "natom": ff.natom, "npair": npair, "ml": meta["ml"], "nmd": meta["nmd"],
           "steps": args.steps, "us_per_step": wall / args.steps * 1e6,
           "device_force_evals_per_step_per_traj": float(st.force_evals().sum() - ev0) / (args.steps * B),
           # algorithmic bytes of one evaluation of all trajectories: q read and Fc written once per
           # DOF and trajectory, Q0 written, the neighbour table (64 B per pair end) and geometry once
           "force_eval_bytes": 3 * 8 * 3 * ff.natom * B + 64 * 2 * npair + 3 * 8 * 3 * ff.natom,
           "q_finite": bool(np.all(np.isfinite(np.asarray(m.q))))}
    m.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", choices=VARIANTS, default=None, help="run one variant in this process")
    ap.add_argument("--ntraj", type=int, default=64)
    ap.add_argument("--steps", type=int, default=512)
    ap.add_argument("--warmup", type=int, default=64)
    ap.add_argument("--ml", type=int, default=None)
    ap.add_argument("--nmd", type=int, default=None)
    ap.add_argument("--limit", type=float, default=300.0, help="seconds per variant")
    args = ap.parse_args()
    if args.variant:
        run_variant(args)
        return 0
    res = {}
    for v in VARIANTS:
        cmd = [sys.executable, os.path.abspath(__file__), "--variant", v, "--ntraj", str(args.ntraj), "--steps",
               str(args.steps), "--warmup", str(args.warmup)]
        for k in ("ml", "nmd"):
            if getattr(args, k) is not None:
                cmd += ["--" + k, str(getattr(args, k))]
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            print("variant %s exceeded %.0f s: stopping" % (v, args.limit), file=sys.stderr)
            return 1
        if r.returncode != 0:
            print("variant %s failed (exit %d): stopping" % (v, r.returncode), file=sys.stderr)
            return 1
        line = r.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        res[v] = json.loads(line)
    us = {v: res[v]["us_per_step"] for v in VARIANTS}
    print(json.dumps({"us_per_step": us, "field_cost_us": us["device"] - us["harmonic"],
                      "gain_over_host": us["host"] / us["device"]}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
