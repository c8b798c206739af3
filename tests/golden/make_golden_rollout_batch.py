#!/usr/bin/env python
"""Yardsticks of the device-resident model rollouts (tests/_rollout_batch_cases.py), on the CPU.

d_<case>: per disagreement case, the distance of a plain fp32 torch restatement -- ((s_next - predict(s, a)) ** 2).mean(-1), the
maximum over the members -- from the fp64 oracle, measured exactly as the GPU worker measures the kernel (row_err).
e2e_roll: for the end-to-end case, the distance of a plain fp32 torch rollout of train_step's draws (policy mean, + noise exp(log_std),
clamp, dynamics, clamp) from the fp64 rollout, per state column relative to the column's largest value (_plan_cases.col_err).
    python tests/golden/make_golden_rollout_batch.py      ->  tests/golden/rollout_batch.npz"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import _plan_cases as C  # noqa: E402
import _rollout_batch_cases as B  # noqa: E402

torch.set_num_threads(1)


def mlp32(theta, sz, x, act):
    o = 0
    for i in range(len(sz) - 1):
        W = theta[o:o + sz[i + 1] * sz[i]].reshape(sz[i + 1], sz[i]); o += W.numel()
        b = theta[o:o + sz[i + 1]]; o += sz[i + 1]
        x = torch.nn.functional.linear(x, W, b)
        if i < len(sz) - 2:
            x = torch.tanh(x) if act == C.TANH else torch.relu(x)
    return x


def e2e_rollout32(o):
    """the end-to-end case's rollout as plain fp32 torch -> obs (K, N, H, n)"""
    e, mem = B.E2E, o["mem"]
    n, m, din = e["n"], e["m"], e["n"] + e["m"]
    models, pol, init, _ = B.e2e_setup()
    pt, ptr = torch.from_numpy(np.float32(pol.get_param_values())), torch.from_numpy(np.float32(pol.model.packed_transforms()))
    noise = torch.from_numpy(o["noise"])
    out = np.zeros((e["K"], e["N"], e["H"], n), np.float32)
    for k in range(e["K"]):
        th, tr = torch.from_numpy(mem["thetas"][k]), torch.from_numpy(mem["trs"][k])
        s = torch.from_numpy(np.float32(init))
        for t in range(e["H"]):
            out[k, :, t] = s.numpy()
            a = mlp32(pt[:-m], o["pol_sizes"], (s - ptr[:n]) / (ptr[n:2 * n] + 1e-8), C.TANH) * ptr[2 * n + m:] + ptr[2 * n:2 * n + m]
            a = torch.clamp(a + noise[k, t] * torch.exp(pt[-m:]), -1e2, 1e2)
            h = mlp32(th, mem["sizes"], (torch.cat([s, a], -1) - tr[:din]) / (tr[din:2 * din] + 1e-8), mem["act"])
            osh, osc = tr[2 * din:2 * din + n], tr[2 * din + n:]
            if mem["flags"] & C.AFF:
                h = h * (osc + 1e-8) + osh
            if mem["flags"] & C.MASK:
                h = h * (osc >= 1e-8)
            if mem["flags"] & C.RES:
                h = h + s
            s = torch.clamp(h, -1e2, 1e2)
    return out


def main():
    out = {}
    for case in B.dis_cases():
        mem, obs, act = B.dis_data(case)
        out["d_" + B.dis_id(case)] = np.float64(B.row_err(B.torch_err32(mem, obs, act), B.oracle_err(mem, obs, act)))
    worst = max(out, key=lambda k: out[k])
    print("%d disagreement cases: fp32 torch is at most %.3e from fp64 (%s); %d are exact" %
          (len(out), out[worst], worst, sum(1 for v in out.values() if v == 0)))
    o = B.e2e_oracle()
    out["e2e_roll"] = np.float64(C.col_err(e2e_rollout32(o)[:, :, 1:], o["obs"][:, :, 1:], np.arange(B.E2E["n"]))[0])
    v = B.first_violation(o["err"], o["lim"])
    print("end to end: the fp32 rollout is %.3e from fp64; lim %.6e truncates %d of %d paths" % (out["e2e_roll"], o["lim"], int(np.sum(v >= 0)), len(v)))
    np.savez(os.path.join(HERE, "rollout_batch.npz"), **out)


if __name__ == "__main__":
    with torch.no_grad():
        main()
