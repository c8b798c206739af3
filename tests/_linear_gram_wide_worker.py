"""GPU worker of tests/test_gpu_linear_gram_wide.py: the wide Gram route (csrc/linear_policy_wide.h: mjx_linear_moments_wide,
mjx_npg_update_linear_wide, mjx_trpo_update_linear_wide) against oracle/npg_oracle.py in fp64, every case once, one RESULT line."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from mjrl_amd._lib import check, ptr  # noqa: E402
from oracle import npg_oracle as O  # noqa: E402
from oracle import synth  # noqa: E402
from tests._linear_gram_trpo_dapg_worker import KL, call  # noqa: E402
from tests._linear_gram_worker import DAMPING, DELTA, ITERS, TOL, Case, fisher_from_G, lib, rel  # noqa: E402
from tests._worker_dev import checked_block, emit, nan_block, same_bits, stream, switch  # noqa: E402

# (n, m, N, TRPO seed): the seeds are fixed on the CPU oracle so that every trial's KL is at least 1e-3 of kl_dist away from it
# (oracle alone: margins 5.2e-2, 3.2e-3, 4.6e-3, 1.3e-3, 4.5e-3, 5.3e-3; all but the fifth backtrack once)
CASES = [(64, 1, 129, 2), (95, 6, 33, 2), (96, 17, 1025, 2), (127, 32, 1500, 0), (111, 8, 4099, 1), (111, 8, 70001, 0)]
MOMENTS_ONLY = (96, 1, 262147)          # pass 1 alone at chains of the full 8 rounds (the oracle's CG on these rows takes too long)


def moments(c):
    L = 96 if c.n < 96 else 128
    cnt = L * L + c.m * L + c.m + 4
    blk = nan_block(cnt, torch.float64)
    check(lib.mjx_linear_moments_wide(c.ctx, ptr(blk), stream()))
    return checked_block(blk, cnt, "moment block"), L


def npg(c, entry=None):
    head = [c.ctx, ITERS, DAMPING, TOL, DELTA, float("nan"), -3.0]
    return call(c, entry or lib.mjx_npg_update_linear_wide, head, routed=entry is None)


def run_moments(n, m, N):
    c = Case(n, m, N, True)
    th, o, a, w = c.o64
    blk, L = moments(c)
    blk2, _ = moments(c)
    G, gWb, rest = blk[:L * L].reshape(L, L) / N, blk[L * L:L * L + m * L].reshape(m, L) / N, blk[L * L + m * L:]
    v = np.random.RandomState(7).randn(c.d)
    g = np.concatenate([gWb[:, :n].ravel(), gWb[:, n], rest[:m] / N])
    out = dict(fvp=rel(fisher_from_G(c, G, L, v), O.fvp(th, o, v, n, m, (), c.otr)), vpg=rel(g, O.vpg(th, th, o, a, w, n, m, (), c.otr, c.otr)),
               surr=abs(rest[m] / N - O.surrogate(th, th, o, a, w, n, m, (), c.otr, c.otr)), rows=rest[m + 1], tail=[rest[m + 2], rest[m + 3]],
               same_bits=same_bits(blk, blk2), pad=float(np.abs(G[n + 1:]).max(initial=0.0) + np.abs(G[:, n + 1:]).max(initial=0.0)
                                                         + np.abs(gWb[:, n + 1:]).max(initial=0.0)))
    return c, out


def run_case(n, m, N, seed):
    c, out = run_moments(n, m, N)
    u = npg(c)
    out.update(route=u["route"], npg=c.errors(u, c.oracle()))
    c.close()
    # TRPO, on its own seed
    c = Case(n, m, N, True, seed=seed)
    th, o, a, w = c.o64
    ref = O.trpo_update(th.copy(), o, a, w, n, m, (), c.otr, cg_iters=ITERS, damping=DAMPING, kl_dist=KL)
    a0 = np.sqrt(abs(2 * KL / (ref["vpg"].dot(ref["npg"]) + 1e-20)))
    kls = [O.mean_kl(th + a0 * 0.9 ** k * ref["npg"], th, o, n, m, (), c.otr, c.otr) for k in range(ref["tries"])]      # (no log_std reaches the clamp)
    assert min(abs(k - KL) / KL for k in kls) >= 1e-3, kls          # the inputs, on the oracle's numbers alone
    u = call(c, lib.mjx_trpo_update_linear_wide, [c.ctx, ITERS, DAMPING, TOL, 2 * KL, KL, 100, -3.0])
    r = u["res"]
    out["trpo"] = dict(route=u["route"], trials=r[11], want_trials=ref["tries"], accepted=r[10], alpha=abs(r[9] - ref["alpha"]) / ref["alpha"],
                       x=rel(u["x"], ref["npg"]), step=rel(u["theta"].astype(np.float64) - th, ref["new_params"] - th),
                       ring=max(abs(r[17 + 2 * k] / N - kl) / kl for k, kl in enumerate(kls)), kl=abs(r[1] / N - ref["kl"]) / ref["kl"])
    c.close()
    return out


def run_once():
    out = {}
    c = Case(111, 8, 4099, True)
    with switch("MJX_LINEAR_GRAM_WIDE", "0"):          # route 0 at n = 111, the bits of mjx_npg_update
        off = npg(c)
    on = npg(c, lib.mjx_npg_update)
    out["switch"] = dict(route=off["route"], same=all(same_bits(off[k], on[k]) for k in ("grad", "x", "theta", "res")))
    c.close()

    # the host classes on a small (70, 3) batch
    from mjrl_amd.algos.dapg import DAPG
    from mjrl_amd.algos.npg_cg import NPG
    from mjrl_amd.policies.gaussian_linear import LinearPolicy

    class Spec:
        observation_dim, action_dim, horizon = 70, 3, 50

    paths = synth.make_paths(4, 50, 70, 3, seed=0)
    for p in paths:
        p["advantages"] = np.random.RandomState(5).randn(len(p["rewards"]))
    routes = {}
    for key, gram in (("wide", "wide"), ("narrow", True)):
        agent = NPG(None, LinearPolicy(Spec, seed=1), None, normalized_step_size=0.05, gram=gram)
        agent.train_from_paths(paths)
        routes[key] = agent.last_update["route"]
        agent.engine.close()
    try:
        DAPG(None, LinearPolicy(Spec, seed=1), None, gram="wide")
        routes["dapg"] = "no error"
    except ValueError:
        routes["dapg"] = "ValueError"
    out["classes"] = routes
    return out


if __name__ == "__main__":
    payload = {"%d_%d_%d" % cs[:3]: run_case(*cs) for cs in CASES}
    c, payload["%d_%d_%d" % MOMENTS_ONLY] = run_moments(*MOMENTS_ONLY)
    c.close()
    payload["once"] = run_once()
    emit(payload)
