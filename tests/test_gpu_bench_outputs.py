"""bench.py's plain run and --dump-outputs: the line holds the headline and ms_per_step and none of the
--full measurements, --steps sets the number of timed steps, and the dumped p / q / f are the state
after the last timed step of trajectories that depend on the arguments alone -- the same benched
system stepped here through md.steps, in this process, arrives at them."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NTRAJ, STEPS, WARMUP = 8, 8, 2


def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def test_plain_run_dumps_the_state_after_the_last_timed_step(tmp_path):
    env = {k: v for k, v in os.environ.items()
           if not k.startswith("GLE_") and k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    out = tmp_path / "dump"
    proc = subprocess.Popen([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--ntraj", str(NTRAJ),
                             "--steps", str(STEPS), "--warmup", str(WARMUP), "--dump-outputs", str(out)],
                            env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=str(tmp_path))
    # the same system as bench.py builds (its seeds), stepped in one go while the benchmark runs
    from sclmd_amd import md as MD
    from sclmd_amd import synthetic

    dyn, axyz, baths, meta = synthetic.junction("C3", seed=1234, gmem_device=True)
    m = MD.md(meta["dt"], meta["nmd"], meta["T"], axyz=axyz, dyn=dyn, ntraj=NTRAJ, seed=1000, traj_offset=0,
              device=0, noise_mode="device", verbose=False)
    try:
        for b in baths:
            m.AddBath(b)
        m.initialise()
        m.ResetHis()
        for i in range(len(baths)):
            m.gen_noise(i, 0)
        st = m._ensure_device()
        ptop = max(P for P, _ in st.profile_levels())
        o, e = proc.communicate(timeout=120)
        assert proc.returncode == 0, o[-2000:] + e[-4000:]
        lines = [ln for ln in o.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, o[-2000:]
        res = json.loads(lines[0])
        assert res["steps"] == STEPS and res["warmup"] == WARMUP and res["n_gpus"] == 1
        assert res["ms_per_step"] > 0 and res["dtype"] == "f64" and res["higher_is_better"] is True
        assert abs(res["value"] - NTRAJ / (res["ms_per_step"] * 1e-3)) <= 1e-9 * res["value"]
        assert not res["full"] and res["window_phase"] is None
        assert not {"roofline", "chain_roofline", "cpu_baseline", "speedup_vs_cpu_baseline"} & set(res)
        # the window starts after the fill and the warm-up, and is STEPS long
        assert res["fill_steps"] == 2 * ptop and res["window_t0"] == 2 * ptop + WARMUP
        m.steps(res["window_t0"] + STEPS)
        p, q, t = st.get_state()
        f = st.get_force()
    finally:
        m.close()
    assert t == res["window_t0"] + STEPS
    assert sorted(os.listdir(out)) == ["f.npy", "p.npy", "q.npy"]
    for name, ref in (("p", p), ("q", q), ("f", f)):
        got = np.load(out / (name + ".npy"))
        assert got.dtype == np.float64 and got.shape == (NTRAJ, meta["nph"]) and np.all(np.isfinite(got))
        assert np.max(np.abs(ref)) > 0
        # fp64 throughout; the same steps in other launch batches (sums may be ordered otherwise)
        assert rel(got, ref) < 1e-9, (name, rel(got, ref))
