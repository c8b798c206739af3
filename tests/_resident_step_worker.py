"""GPU worker for tests/test_gpu_resident_train_step.py: ModelAccelNPG.train_step on the resident route against the host route, in ONE
fresh process; prints one JSON line of what it found (the test module holds the bars).  The end-to-end case and its truncation limit
come from tests/_rollout_batch_cases.py (e2e_setup, e2e_oracle).  python tests/_resident_step_worker.py"""
import contextlib
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import _plan_cases as C  # noqa: E402
import _rollout_batch_cases as B  # noqa: E402
from mjrl_amd.algos.model_accel import model_accel_npg as A  # noqa: E402
from mjrl_amd.algos.model_accel import nn_dynamics as D  # noqa: E402
from mjrl_amd.baselines.linear_baseline import LinearBaseline  # noqa: E402
from mjrl_amd.policies.gaussian_mlp import MLP  # noqa: E402
from mjrl_amd.utils import ingest  # noqa: E402
from tests._worker_dev import emit, switch  # noqa: E402

R = {}
SWITCHES = ("MJX_POLICY_ROLLOUT_MFMA", "MJX_PATH_REWARDS_MFMA", "MJX_ROLLOUT_DISAGREE_MFMA")
KEYS = ("observations", "actions", "rewards", "returns", "advantages")
LIM = B.e2e_oracle()["lim"]


class Env:
    def __init__(self, spec):
        self.horizon, self.spec = spec.horizon, spec
        self.observation_dim, self.action_dim = spec.observation_dim, spec.action_dim

    def reset(self):
        return np.zeros(self.observation_dim)

    def set_seed(self, seed=None):
        pass


def reward_function(paths):
    paths["rewards"] = -np.sum(paths["observations"] ** 2, -1) - 0.1 * np.sum(paths["actions"] ** 2, -1)
    return paths


def step(resident, forced0=False, learn_reward=True, change=None, truncate_lim=LIM, warm=None, **kw):
    """one train_step of a fresh agent from the case's seeds -> dict(paths, stats, keys, theta, info) or dict(raised).  warm (a
    callable): a first step fits the baseline, then warm() is called and the step that counts follows"""
    models, pol, init, spec = B.e2e_setup(learn_reward)
    if change is not None:
        spec = change(models, spec) or spec
    env = Env(spec)
    if not all(mdl.learn_reward for mdl in models):
        kw.setdefault("reward_function", reward_function)
    agent = A.ModelAccelNPG(learned_model=models, env=env, policy=pol, baseline=LinearBaseline(env.spec), normalized_step_size=0.05, seed=9,
                            save_logs=True, **kw)
    got, fit0 = [], agent.baseline.fit

    def fit(paths, return_errors=False):
        got.extend(dict({k: np.array(p[k]) for k in KEYS}, terminated=bool(p["terminated"])) for p in paths)
        return fit0(paths, return_errors=return_errors)

    agent.baseline.fit = fit
    call = lambda: agent.train_step(B.E2E["N"], env=env, init_states=[x for x in init], truncate_lim=truncate_lim,   # noqa: E731
                                    truncate_reward=-1.0, resident=resident)
    with contextlib.ExitStack() as held:
        for s in SWITCHES:
            held.enter_context(switch(s, "0" if forced0 else None))
        if warm is not None:
            call()
            del got[:]
            warm()
        torch.manual_seed(B.E2E["noise_seed"])          # (the draws e2e_oracle fixed the limit on)
        try:
            stats = call()
        except Exception as e:                         # (compared between the routes by the caller)
            return dict(raised=type(e).__name__, info=agent.train_step_info())
        finally:
            ingest.drop_shared_batch()
    return dict(paths=got, stats=[float(v) for v in stats], keys=sorted(agent.logger.log.keys()), theta=pol.get_param_values().astype(np.float64),
                info=agent.train_step_info())


def same_paths(a, b):
    """array for array: values, dtypes, lengths, terminated -> the list of what differs"""
    bad = []
    if len(a) != len(b):
        return ["count %d != %d" % (len(a), len(b))]
    for k in KEYS:
        if any(p[k].dtype != q[k].dtype or p[k].shape != q[k].shape for p, q in zip(a, b)):
            bad.append(k + ": dtype or shape")
        elif any(not np.array_equal(p[k], q[k]) for p, q in zip(a, b)):
            bad.append(k + ": values")
    if [p["terminated"] for p in a] != [q["terminated"] for q in b]:
        bad.append("terminated")
    return bad


def lens(r):
    return [len(p["rewards"]) for p in r["paths"]]


# ---- (a) every route switch forced to 0: the resident step against the host route, and two host runs against each other
h1, h2, r0 = step(False, True), step(False, True), step(True, True)
R["a_info"] = r0["info"]
R["a_host_info"] = h1["info"]
R["a_paths"] = same_paths(r0["paths"], h1["paths"])
R["a_stats"] = [r0["stats"], h1["stats"]]
R["a_keys"] = [r0["keys"], h1["keys"]]
R["a_theta"] = [float(np.max(np.abs(r0["theta"] - h1["theta"]))), float(np.max(np.abs(h2["theta"] - h1["theta"])))]
R["a_truncated"] = [int(sum(p["terminated"] for p in h1["paths"])), len(h1["paths"]), min(lens(h1)), max(lens(h1))]

# ---- (b) default routes
r1 = step(True)
R["b_info"] = r1["info"]
R["b_lens"] = [lens(r1) == lens(r0), [p["terminated"] for p in r1["paths"]] == [p["terminated"] for p in r0["paths"]]]
if R["b_lens"][0]:
    oa, ob = np.concatenate([p["observations"] for p in r0["paths"]]), np.concatenate([p["observations"] for p in r1["paths"]])
    R["b_obs"] = [C.col_err(ob, oa, np.arange(B.E2E["n"]))[0], float(np.load(B.FIXTURE)["e2e_roll"])]
    R["b_differs"] = bool(np.any(oa != ob))

# ---- (c) learned rewards: nothing of the batch's row count goes up during the resident step
seen = []
up0, stage0, add0 = ingest.upload, ingest.PathStager.stage, ingest.PathStager.add_paths


def rows_of(paths):
    return [int(sum(len(p[k]) for p in paths)) for k in paths[0] if isinstance(paths[0][k], np.ndarray)] if paths else []


def upload(backend, a, dtype=None):
    seen.append(("upload", [int(np.shape(a)[0])] if np.ndim(a) else []))
    return up0(backend, a, dtype)


def stage(self, paths, *args, **kw):
    seen.append(("stage", rows_of(paths)))
    return stage0(self, paths, *args, **kw)


def add_paths(self, paths):
    seen.append(("add_paths", rows_of(paths)))
    return add0(self, paths)


ingest.upload, ingest.PathStager.stage, ingest.PathStager.add_paths = upload, stage, add_paths
try:
    rc = step(True, warm=lambda: seen.clear())      # (an unfitted baseline predicts zeros on the host: the second step counts)
    rows = rc["info"]["rows"]
    R["c_resident"] = [rows, [s for s in seen if rows in s[1]]]
    hc = step(False, warm=lambda: seen.clear())
    hrows = sum(lens(hc))
    R["c_host"] = [hrows, len([s for s in seen if hrows in s[1]])]
finally:
    ingest.upload, ingest.PathStager.stage, ingest.PathStager.add_paths = up0, stage0, add0

# ---- (d) the reference's fixture (host reward_function, ts_trunc): lengths and statistics
G = np.load(os.path.join(ROOT, "tests", "golden", "model_accel.npz"))
n, m = 6, 2
models = []
for k in range(3):
    wm = D.WorldModel(n, m, hidden_size=(32, 32), seed=70 + k)
    th, tr = G["ts_model%d" % k], G["ts_model%d_tr" % k]
    ws, o = [], 0
    for p in wm.dynamics_net.parameters():
        ws.append(torch.from_numpy(th[o:o + p.numel()].reshape(p.shape).copy())); o += p.numel()
    trs = [torch.from_numpy(tr[o:o + l].copy()) for o, l in zip(np.cumsum([0, n, n, m, m, n]), [n, n, m, m, n, n])]
    wm.dynamics_net.set_params(dict(weights=ws, transforms=trs))
    models.append(wm)
env = Env(types.SimpleNamespace(observation_dim=n, action_dim=m, horizon=12))
pol = MLP(env.spec, hidden_sizes=(8, 8), seed=4, init_log_std=-0.5)
agent = A.ModelAccelNPG(learned_model=models, env=env, policy=pol, baseline=LinearBaseline(env.spec), normalized_step_size=0.05, seed=9,
                        save_logs=True, reward_function=reward_function, resident=True)
flens, fit0 = [], agent.baseline.fit


def fit(paths, return_errors=False):
    flens.extend(len(p["rewards"]) for p in paths)
    return fit0(paths, return_errors=return_errors)


agent.baseline.fit = fit
torch.manual_seed(81)
stats = np.array(agent.train_step(40, env=env, init_states=[x for x in G["ts_init"]], truncate_lim=float(G["ts_trunc"]), truncate_reward=-1.0), np.float64)
R["d_info"] = agent.train_step_info()
R["d_lens"] = bool(np.array_equal(np.array(flens), G["ts_lens"]))
R["d_stats"] = float(np.max(np.abs(stats - G["ts_stats"])) / max(1.0, float(np.max(np.abs(G["ts_stats"])))))
R["d_keys"] = [sorted(agent.logger.log.keys()), sorted(G["ts_keys"].tolist())]
ingest.drop_shared_batch()


# ---- (e) every decline reason: resident False with its why, and the host route's result
def tanh_member(models, spec):
    models[1].dynamics_net.nonlinearity = torch.tanh
    models[1].reward_net.nonlinearity = torch.tanh


def mixed(models, spec):
    models[2].learn_reward = False


def short(models, spec):
    return types.SimpleNamespace(observation_dim=spec.observation_dim, action_dim=spec.action_dim, horizon=4)


def outcome(r):
    return r["raised"] if "raised" in r else [r["stats"], lens(r), float(np.max(np.abs(r["theta"])))]


R["e"] = {}
for name, why, kw, patch in (("termination_function", "termination_function", dict(termination_function=lambda paths: paths), None),
                             ("members_differ", "members differ", dict(change=tanh_member), None),
                             ("mixed_rewards", "mixed rewards", dict(change=mixed), None),
                             ("short_horizon", "horizon < 5", dict(change=short), None),
                             ("distributed", "distributed", {}, "_distributed"),
                             ("no_gpu", "no gpu", {}, "_gpu_available")):
    host = step(False, **kw)
    saved = getattr(A, patch) if patch else None
    if patch:
        setattr(A, patch, (lambda: True) if patch == "_distributed" else (lambda: False))
    try:
        res = step(True, **kw)
    finally:
        if patch:
            setattr(A, patch, saved)
    R["e"][name] = dict(info=res["info"], why=why, same=outcome(res) == outcome(host), host=("raised" in host))
R["f_info"] = step(None)["info"]
emit(R)
