"""Worker of tests/test_gpu_dispatch_matrix.py: runs a list of cases through the layer-wise path with whatever MJX_* switches
the parent set in the environment (some are read once per process) and writes one .npz of device results per case.

    python _dispatch_matrix_worker.py <spec.json> <out_dir>

spec.json: {"kind": "head" | "cg", "cases": [{...}, ...]}.  The inputs are rebuilt from the case's seed by head_inputs() /
cg_inputs(), which the parent calls too (for the fp64 oracle)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import npg_oracle as O  # noqa: E402
from oracle import synth  # noqa: E402
from tests._lw_check import out_layer_offsets  # noqa: E402


def probe_actions(m):
    return sorted({a for a in (0, m - 2, m - 1) if a >= 0})


def probe_direction(v, n, m, hid, a):
    """v restricted to output row a: its weight row W3[a, :] and bias entry b3[a], zero elsewhere"""
    h = hid[-1]
    oW, ob = out_layer_offsets(n, m, hid)
    p = np.zeros_like(v)
    p[oW + a * h:oW + (a + 1) * h] = v[oW + a * h:oW + (a + 1) * h]
    p[ob + a] = v[ob + a]
    return p


def _pack(tr):
    return np.concatenate([tr.in_shift, tr.in_scale, tr.out_shift, tr.out_scale]).astype(np.float32)


def head_inputs(n, m, hid, N, seed):
    """Inputs under which a misplaced action shows: every action has its own log_std, out_scale and out_shift (permuted, so
    neighbours differ), non-identity input transforms, on-policy actions (z ~ N(0, 1) for every action)."""
    rng = np.random.RandomState(seed)
    th = synth.perturbed_params(synth.init_params(n, m, hid), scale=0.05)
    th[-m:] = np.linspace(-1.5, 0.5, m)[rng.permutation(m)]
    tr = O.Transforms(n, m, 0.1 * rng.randn(n), 1 + 0.1 * rng.rand(n), np.linspace(-0.3, 0.3, m)[rng.permutation(m)],
                      np.linspace(0.6, 1.4, m)[rng.permutation(m)])
    obs = rng.randn(N, n).astype(np.float32)
    mu = O.forward(th.astype(np.float64), obs.astype(np.float64), n, m, hid, tr)
    act = (mu + np.exp(th[-m:].astype(np.float64)) * rng.randn(N, m)).astype(np.float32)
    adv = rng.randn(N).astype(np.float32)
    # (the old network of K1 / K3: per-weight noise scaled down with the width, as in test_other_shapes_vs_oracle)
    th2 = (th + 0.02 * (64.0 / max([64] + list(hid))) * rng.randn(th.size)).astype(np.float32)
    v = rng.randn(th.size).astype(np.float32)
    return dict(th=th, th2=th2, tr=tr, pk=_pack(tr), obs=obs, act=act, adv=adv, v=v)


def cg_inputs(n, m, hid, N, seed):
    """Every log_std starts just above the clamp min_log_std = -0.5 (a step may push it below); on-policy actions, whitened
    advantages (what npg_update expects)."""
    rng = np.random.RandomState(seed)
    th = synth.perturbed_params(synth.init_params(n, m, hid), scale=0.05)
    th[-m:] = -0.4999
    tr = O.Transforms(n, m, 0.1 * rng.randn(n), 1 + 0.1 * rng.rand(n), 0.05 * rng.randn(m), 1 + 0.2 * rng.rand(m))
    obs = rng.randn(N, n).astype(np.float32)
    mu = O.forward(th.astype(np.float64), obs.astype(np.float64), n, m, hid, tr)
    act = (mu + np.exp(th[-m:].astype(np.float64)) * rng.randn(N, m)).astype(np.float32)
    adv = O.whiten(rng.randn(N)).astype(np.float32)
    th0 = th.copy()
    th0[-m] = -0.75                   # (the iters = 0 update: one log_std below the clamp, the only entry that may move)
    return dict(th=th, th0=th0, tr=tr, pk=_pack(tr), obs=obs, act=act, adv=adv)


def _engine(n, m, hid):
    from mjrl_amd.engine import UpdateEngine
    eng = UpdateEngine(n, m, tuple(hid))
    assert not eng.fused, "MJX_FORCE_LAYERWISE=1 expected in the worker's environment"
    return eng


def run_head(c):
    import torch
    n, m, hid, N = c["n"], c["m"], tuple(c["hid"]), c["N"]
    inp = head_inputs(n, m, hid, N, c["seed"])
    th, th2, pk = inp["th"], inp["th2"], inp["pk"]
    eng = _engine(n, m, hid)
    out = {}
    eng.set_policy(th, th, pk, pk)
    eng.set_batch(inp["obs"], inp["act"], inp["adv"])
    g, surr = eng.surr_vpg()
    out["g"], out["surr"] = g.cpu().numpy().copy(), surr
    dev = lambda a: torch.from_numpy(a).to(eng.device)
    out["hv"] = eng.fvp(dev(inp["v"])).cpu().numpy().copy()
    for a in probe_actions(m):
        out["hv_a%d" % a] = eng.fvp(dev(probe_direction(inp["v"], n, m, hid, a))).cpu().numpy().copy()
    eng.set_policy(th2, th, pk, pk)
    out["s"], out["kl"] = eng.eval_surr_kl()
    out["g2"] = eng.surr_vpg()[0].cpu().numpy().copy()
    eng.close()
    return out


def run_cg(c):
    n, m, hid, N = c["n"], c["m"], tuple(c["hid"]), c["N"]
    inp = cg_inputs(n, m, hid, N, c["seed"])
    th, pk, damping = inp["th"], inp["pk"], c["damping"]
    eng = _engine(n, m, hid)
    out = {"d": eng.d}
    eng.set_policy(th, th, pk, pk)
    eng.set_batch(inp["obs"], inp["act"], inp["adv"])
    g, _ = eng.surr_vpg()
    out["g"] = g.cpu().numpy().copy()
    for it in (0, 1, 10):
        x, bx = eng.cg_solve(g, it, damping)
        out["x%d" % it], out["bx%d" % it] = x.cpu().numpy().copy(), bx
    x, bx = eng.cg_solve(g, 12, c["brk_damping"], tol=c["brk_tol"])
    out["xbrk"] = x.cpu().numpy().copy()
    for tag, t0, it in (("upd", th, 10), ("upd0", inp["th0"], 0)):
        eng.set_policy(t0, t0, pk, pk)
        eng.set_batch(inp["obs"], inp["act"], inp["adv"])
        surr_after, kl = eng.npg_update(it, damping, c["step_size"], c["min_log_std"])
        late = eng.deferred()
        out[tag + "_x"] = eng.x.cpu().numpy().copy()
        out[tag + "_theta"] = eng.theta_new.cpu().numpy().copy()
        out[tag + "_alpha"], out[tag + "_gdotx"] = late["alpha"], late["gdotx"]
        out[tag + "_surr_before"], out[tag + "_surr_after"], out[tag + "_kl"] = late["surr_before"], surr_after, kl
    eng.close()
    return out


def main():
    spec_path, out_dir = sys.argv[1], sys.argv[2]
    with open(spec_path) as f:
        spec = json.load(f)
    run = run_head if spec["kind"] == "head" else run_cg
    for c in spec["cases"]:
        np.savez(os.path.join(out_dir, c["name"] + ".npz"), **run(c))


if __name__ == "__main__":
    main()
