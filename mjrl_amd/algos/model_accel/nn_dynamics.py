"""Learned dynamics / reward models on the GPU.

Mirrors ``mjrl.algos.model_accel.nn_dynamics`` (reference nn_dynamics.py:7-385): the same classes, constructor
arguments, parameters (torch ``nn.Linear`` layers built after ``torch.manual_seed(seed)``, so the initial weights and the
global torch stream are the reference's) and transforms.  What runs where:

* ``forward`` / ``predict`` / ``reward`` / ``compute_loss``: the batched forward kernel (``mjx_dyn_forward``), K ensemble
  members per launch through :func:`ensemble_forward`;
* ``fit_dynamics`` / ``fit_reward``: the transforms are formed with the reference's torch expressions, the epoch
  permutations are drawn from NumPy's global stream exactly where ``fit_model`` draws them, and every Adam step runs in
  libmjx (``mjx_dyn_fit_adam``: one persistent launch for nets up to 128 wide at minibatch <= 64, a launch per layer and
  phase otherwise).  The optimiser state (``dynamics_opt`` / ``reward_opt``) is torch.optim.Adam's -- step count and
  both moments -- kept as flat fp32 vectors;
* :func:`fit_ensemble`: the driver's ``for model in ensemble: model.fit_dynamics(...)`` with every member's Adam chain in one
  persistent launch (``mjx_dyn_fit_ensemble``, a workgroup per member on fp32 MFMAs for two hidden layers up to 256 wide);
* :func:`fit_reward_ensemble`: the same for the K reward nets (``mjx_reward_fit_ensemble``: any two hidden widths up to 256, the
  loss through the output affine); :func:`fit_world_models`: the driver's interleaved loop (dynamics, reward, next member) as
  two such calls; :func:`ensemble_path_rewards`: every member's ``compute_path_rewards`` in one upload, two launches and one
  read-back; :func:`ensemble_path_rewards_device`: the same on device tensors in one ``mjx_path_rewards`` call, which is what
  ``MPCPolicy(reward='learned')`` plans on;
* :func:`rollout_disagreement_device`: the ensemble-disagreement error of rollouts that are on the device
  (``mjx_rollout_disagreement``), which ``ModelAccelNPG.train_step(resident=True)`` truncates on.  Both device passes take
  ``wide=True``: for dynamics nets wider than 128 (:func:`wide_rows_shape`) they then call the ``_wide`` entries
  (csrc/rows_wide.h: fp32 MFMAs for nets up to 256 wide, route 2).

What every one of these shares stands once: :func:`pack_members` (K nets of one shape as the device blocks ``P`` and ``tr``, under
every forward, rollout, fit and under ``pack_dynamics_members`` / ``pack_reward_members``), :func:`_dynamics_transforms` /
:func:`_reward_transforms` (the reference's transform expressions), :func:`_fit_members` (the one fit body: index draws, X, stacked
state, the entry, :func:`_write_back`) and :func:`cached_members_pack` (the device cache of a planner's members, keyed by
:func:`members_pack_key`).

The module parameters stay ordinary torch tensors (CPU by default, as in the reference): ``get_params`` /
``set_params`` / ``to`` / ``is_cuda`` / pickling behave as the reference's.  There is no CPU path: without a GPU the
operations raise.
"""
import ctypes
import os

import numpy as np
import torch
import torch.nn as nn

from ..._lib import MjxError, check, load, ptr

ACT_RELU, ACT_TANH = 0, 1
OUT_AFFINE, MASK, RESIDUAL = 1, 2, 4
TGT_AFFINE, TGT_PLAIN, TGT_RESIDUAL = 0, 1, 2


def _device():
    if not torch.cuda.is_available():
        raise MjxError("model_accel: no GPU visible -- the learned-model operations run in libmjx only")
    return torch.device("cuda", torch.cuda.current_device())


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _ints(v):
    return (ctypes.c_int * len(v))(*[int(x) for x in v])


def _f32(x, dev):
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(x)
    return x.to(device=dev, dtype=torch.float32).contiguous()


def _act_code(net):
    return ACT_TANH if net.nonlinearity is torch.tanh else ACT_RELU


def _flat_params(net, dev):
    return torch.cat([p.detach().reshape(-1).to(dev, torch.float32) for p in net.parameters()])


def _vec(v, k):
    if isinstance(v, torch.Tensor):
        v = v.detach().to("cpu", torch.float32).reshape(-1)
        return v.expand(k) if v.numel() == 1 else v
    return torch.full((k,), float(v), dtype=torch.float32)


def _packed_transforms(net, dev):
    """[in_shift, in_scale, out_shift, out_scale] over the concatenated input (csrc/dynamics.h)"""
    if isinstance(net, RewardNet):
        sh = [net.s_shift, net.a_shift, net.sp_shift]
        sc = [net.s_scale, net.a_scale, net.sp_scale]
        k = 1
    else:
        sh, sc, k = [net.s_shift, net.a_shift], [net.s_scale, net.a_scale], net.out_dim
    ins = [_vec(v, v.numel()) for v in sh] + [_vec(v, v.numel()) for v in sc]
    return torch.cat(ins + [_vec(net.out_shift, k), _vec(net.out_scale, k)]).to(dev)


def _flags(net):
    if isinstance(net, RewardNet):
        return OUT_AFFINE
    if not net._apply_out_transforms:
        return 0
    return OUT_AFFINE | (MASK if net.use_mask else 0) | (RESIDUAL if net.residual else 0)


def _one_shape(nets):
    sizes = tuple(nets[0].layer_sizes)
    assert all(tuple(net.layer_sizes) == sizes for net in nets), "ensemble members must share one shape"
    return sizes


def _stack(blocks):
    """K blocks as K rows; one block is its own row (a view: what writes to the row writes to the block)"""
    return blocks[0][None] if len(blocks) == 1 else torch.stack(blocks)


def pack_members(nets, dev, one_kind=True):
    """THE packer: K nets of one shape (asserted) as the device blocks every entry reads -> dict(sizes, P (K x params), tr (K x
    transforms, :func:`_packed_transforms`), act, flags).  ``one_kind``: the nets share (activation, flags) as well (asserted), as a
    launch over all of them needs; without it ``act`` and ``flags`` are the first net's."""
    sizes = _one_shape(nets)
    assert not one_kind or len({(_act_code(net), _flags(net)) for net in nets}) == 1, "ensemble members must share activation and output transforms"
    return dict(sizes=sizes, P=_stack([_flat_params(net, dev) for net in nets]), tr=_stack([_packed_transforms(net, dev) for net in nets]),
                act=_act_code(nets[0]), flags=_flags(nets[0]))


def ensemble_forward(nets, x, dev=None):
    """K nets of one shape over the same rows x (rows x d_in, the concatenated raw input) in one launch -> K x rows x d_out
    (device tensor).  Each net's own activation, transforms and flags apply (one launch per distinct (activation, flags)).
    x of shape K x rows x d_in: member k reads its own rows x[k] (a per-member x_stride)."""
    dev = dev or _device()
    x = _f32(x, dev)
    own = x.dim() == 3
    assert not own or x.shape[0] == len(nets), "per-member rows: one block per net"
    rows = x.shape[-2]
    sizes = _one_shape(nets)
    out = torch.empty((len(nets), rows, sizes[-1]), dtype=torch.float32, device=dev)
    groups = {}
    for i, net in enumerate(nets):
        groups.setdefault((_act_code(net), _flags(net)), []).append(i)
    lib = load()
    for (act, flags), ids in groups.items():
        pk = pack_members([nets[i] for i in ids], dev)
        o = out if len(ids) == len(nets) else torch.empty((len(ids), rows, sizes[-1]), dtype=torch.float32, device=dev)
        xg = x if not own or len(ids) == len(nets) else x[ids].contiguous()
        check(lib.mjx_dyn_forward(ptr(xg), rows * sizes[0] if own else 0, rows, len(ids), _ints(sizes), len(sizes), ptr(pk["P"]), ptr(pk["tr"]), act, flags,
                                  ptr(o), _stream(dev)))
        if o is not out:
            out[ids] = o
    return out


class _DeviceAdam:
    """torch.optim.Adam(net.parameters(), lr, weight_decay) for one net: step count and flat fp32 moments (on the GPU
    while fitting; ``to`` moves them)."""

    def __init__(self, net, lr=1e-3, weight_decay=0.0):
        self.param_groups = [dict(lr=lr, weight_decay=weight_decay, betas=(0.9, 0.999), eps=1e-8, amsgrad=False)]
        self.num_params = int(sum(p.numel() for p in net.parameters()))
        self.step_count = 0
        self.exp_avg = self.exp_avg_sq = None

    def to(self, device):
        if self.exp_avg is not None:
            self.exp_avg, self.exp_avg_sq = self.exp_avg.to(device), self.exp_avg_sq.to(device)
        return self

    def _state(self, dev):
        if self.exp_avg is None:
            self.exp_avg = torch.zeros(self.num_params, dtype=torch.float32, device=dev)
            self.exp_avg_sq = torch.zeros(self.num_params, dtype=torch.float32, device=dev)
        self.to(dev)
        return self.exp_avg, self.exp_avg_sq


def _dynamics_transforms(residual, s, a, sp):
    """the reference's transform expressions for a dynamics net (nn_dynamics.py:99-104) on tensors of one device -> the six
    arguments of ``DynamicsNet.set_transformations``"""
    s_shift, a_shift = torch.mean(s, dim=0), torch.mean(a, dim=0)
    s_scale, a_scale = torch.mean(torch.abs(s - s_shift), dim=0), torch.mean(torch.abs(a - a_shift), dim=0)
    out_shift = torch.mean(sp - s, dim=0) if residual else torch.mean(sp, dim=0)
    out_scale = torch.mean(torch.abs(sp - s - out_shift), dim=0) if residual else torch.mean(torch.abs(sp - out_shift), dim=0)
    return s_shift, s_scale, a_shift, a_scale, out_shift, out_scale


def _reward_transforms(s, a, r):
    """the reference's transform expressions for a reward net (nn_dynamics.py:135-139) on tensors of one device -> the six arguments
    of ``RewardNet.set_transformations``.  As the reference writes it, the last pair reads ``r_shift`` before it is bound: it
    raises ``UnboundLocalError`` there and here, so reward fits are run with ``set_transformations=False``."""
    s_shift, a_shift = torch.mean(s, dim=0), torch.mean(a, dim=0)
    s_scale, a_scale = torch.mean(torch.abs(s - s_shift), dim=0), torch.mean(torch.abs(a - a_shift), dim=0)
    r_shift, r_scale = torch.mean(r, dim=0), torch.mean(torch.abs(r - r_shift), dim=0)
    return s_shift, s_scale, a_shift, a_scale, r_shift, r_scale


class WorldModel:
    def __init__(self, state_dim, act_dim,
                 learn_reward=False,
                 hidden_size=(64, 64),
                 seed=123,
                 fit_lr=1e-3,
                 fit_wd=0.0,
                 device='cpu',
                 activation='relu',
                 residual=True,
                 *args,
                 **kwargs,):
        """Arguments as in the reference (nn_dynamics.py:8-38)."""
        self.state_dim, self.act_dim = state_dim, act_dim
        self.device, self.learn_reward = device, learn_reward
        if self.device == 'gpu':
            self.device = 'cuda'
        self.dynamics_net = DynamicsNet(state_dim, act_dim, hidden_size, residual=residual, seed=seed).to(self.device)
        self.dynamics_net.set_transformations()
        if activation == 'tanh':
            self.dynamics_net.nonlinearity = torch.tanh
        self.dynamics_opt = _DeviceAdam(self.dynamics_net, lr=fit_lr, weight_decay=fit_wd)
        self.dynamics_loss = torch.nn.MSELoss()
        if self.learn_reward:
            self.reward_net = RewardNet(state_dim, act_dim, hidden_size=(100, 100), seed=seed).to(self.device)
            self.reward_net.set_transformations()
            if activation == 'tanh':
                self.reward_net.nonlinearity = torch.tanh
            self.reward_opt = _DeviceAdam(self.reward_net, lr=fit_lr, weight_decay=fit_wd)
            self.reward_loss = torch.nn.MSELoss()
        else:
            self.reward_net, self.reward_opt, self.reward_loss = None, None, None

    def to(self, device):
        self.dynamics_net.to(device)
        self.dynamics_opt.to(device)
        if self.learn_reward:
            self.reward_net.to(device)
            self.reward_opt.to(device)

    def is_cuda(self):
        return next(self.dynamics_net.parameters()).is_cuda

    def forward(self, s, a):
        if type(s) == np.ndarray:
            s = torch.from_numpy(s).float()
        if type(a) == np.ndarray:
            a = torch.from_numpy(a).float()
        return self.dynamics_net.forward(s.to(self.device), a.to(self.device))

    def predict(self, s, a):
        s = torch.from_numpy(s).float()
        a = torch.from_numpy(a).float()
        return self.dynamics_net.forward(s, a).to('cpu').data.numpy()

    def reward(self, s, a):
        if not self.learn_reward:
            print("Reward model is not learned. Use the reward function from env.")
            return None
        if type(s) == np.ndarray:
            s = torch.from_numpy(s).float()
        if type(a) == np.ndarray:
            a = torch.from_numpy(a).float()
        s, a = s.to(self.device), a.to(self.device)
        sp = self.dynamics_net.forward(s, a).detach().clone()
        return self.reward_net.forward(s, a, sp)

    def compute_loss(self, s, a, s_next):
        # (logging only, as in the reference)
        sp = self.forward(s, a)
        s_next = torch.from_numpy(s_next).float() if type(s_next) == np.ndarray else s_next
        loss = self.dynamics_loss(sp, s_next.to(sp.device))
        return loss.to('cpu').data.numpy()

    def fit_dynamics(self, s, a, sp, fit_mb_size, fit_epochs, max_steps=1e4,
                     set_transformations=True, *args, **kwargs):
        assert type(s) == type(a) == type(sp)
        assert s.shape[0] == a.shape[0] == sp.shape[0]
        if type(s) == np.ndarray:
            s = torch.from_numpy(s).float()
            a = torch.from_numpy(a).float()
            sp = torch.from_numpy(sp).float()
        s = s.to(self.device); a = a.to(self.device); sp = sp.to(self.device)
        net = self.dynamics_net
        if set_transformations:                  # (on the reference's device)
            net.set_transformations(*_dynamics_transforms(net.residual, s, a, sp))
        # targets (sp [- s] - out_shift) / (out_scale + 1e-8) are formed on the GPU (k_dyn_prep); the fit runs in the
        # transformed space (the reference's _apply_out_transforms = False, nn_dynamics.py:107-115)
        return _fit(net, self.dynamics_opt, torch.cat([s, a], -1), sp, TGT_RESIDUAL if net.residual else TGT_PLAIN,
                    fit_mb_size, fit_epochs, max_steps)

    def fit_reward(self, s, a, r, fit_mb_size, fit_epochs, max_steps=1e4,
                   set_transformations=True, *args, **kwargs):
        if not self.learn_reward:
            print("Reward model was not initialized to be learnable. Use the reward function from env.")
            return None
        assert type(s) == type(a) == type(r)
        assert len(r.shape) == 2 and r.shape[1] == 1
        assert s.shape[0] == a.shape[0] == r.shape[0]
        if type(s) == np.ndarray:
            s = torch.from_numpy(s).float()
            a = torch.from_numpy(a).float()
            r = torch.from_numpy(r).float()
        s = s.to(self.device); a = a.to(self.device); r = r.to(self.device)
        if set_transformations:
            self.reward_net.set_transformations(*_reward_transforms(s, a, r))
        sp = self.dynamics_net.forward(s, a).detach().clone()
        sp = sp.to(s.device)
        return _fit(self.reward_net, self.reward_opt, torch.cat([s, a, sp], -1), r, TGT_AFFINE, fit_mb_size, fit_epochs,
                    max_steps)

    def compute_path_rewards(self, paths):
        if not self.learn_reward:
            print("Reward model is not learned. Use the reward function from env.")
            return None
        s, a = paths['observations'], paths['actions']
        num_traj, horizon, s_dim = s.shape
        a_dim = a.shape[-1]
        r = self.reward(s.reshape(-1, s_dim), a.reshape(-1, a_dim))
        paths['rewards'] = r.to('cpu').data.numpy().reshape(num_traj, horizon)


def fit_permutations(num_samples, batch_size, epochs, max_steps=1e10):
    """fit_model's host side (nn_dynamics.py:363-384): one np.random.permutation(num_samples) per epoch, (N // batch) steps
    per epoch, stop after the epoch whose steps reach max_steps -> (row indices of every step, steps per epoch, epochs run)"""
    num_steps = int(num_samples // batch_size)
    idx, steps_so_far, ran = [], 0, 0
    for ep in range(epochs):
        perm = np.random.permutation(num_samples)
        idx.append(perm[:num_steps * batch_size])
        ran += 1
        steps_so_far += num_steps
        if steps_so_far >= max_steps:
            print("Number of grad steps exceeded threshold. Terminating early..")
            break
    flat = np.concatenate(idx).astype(np.int32) if idx else np.zeros(0, np.int32)
    return flat, num_steps, ran


def epoch_means(step_losses, num_steps, epochs):
    """the reference's per-epoch bookkeeping on fp32 losses (`ep_loss += loss.numpy()`, then `ep_loss * 1.0 / num_steps`)"""
    out = []
    for ep in range(epochs):
        ep_loss = 0.0
        for mb in range(num_steps):
            ep_loss += np.array(step_losses[ep * num_steps + mb], dtype=np.float32)
        out.append(ep_loss * 1.0 / num_steps)
    return out


def _write_back(nets, opts, P, m, v, steps, losses, num_steps, ran):
    """THE write-back of a fit: per member the moments and parameters copied back, the optimiser advanced, ``_generation`` bumped
    (``p.data.copy_`` leaves ``p._version`` as it was; holders of device copies key on the counter) -> K epoch-loss lists"""
    out = []
    with torch.no_grad():
        for i, (net, opt) in enumerate(zip(nets, opts)):
            if m.shape[0] > 1:                   # (a single member's moments were updated in place, see _stack)
                opt.exp_avg.copy_(m[i]); opt.exp_avg_sq.copy_(v[i])
            opt.step_count += steps
            k = 0
            for p in net.parameters():
                p.data.copy_(P[i, k:k + p.numel()].view_as(p))
                k += p.numel()
            net._generation = getattr(net, "_generation", 0) + 1
            out.append(epoch_means(losses[i], num_steps, ran))
    return out


def _fit_members(nets, opts, make_x, Y, target_mode, batch_size, epochs, max_steps, entry, draws=None):
    """THE fit body: K nets (one shape, activation and optimiser setting) on N rows through ``entry`` -- ``mjx_dyn_fit_adam`` (K = 1),
    ``mjx_dyn_fit_ensemble`` or ``mjx_reward_fit_ensemble``.  The index draws (``draws``, or member by member from NumPy's global
    stream here), then ``make_x(dev)`` -> (X on the device, its member stride), then the members' parameters, transforms and
    optimiser state stacked, the call, the write-back.  -> K epoch-loss lists."""
    dev = _device()
    K, N = len(nets), int(Y.shape[0])
    idx, num_steps, ran = draws if draws is not None else ensemble_fit_indices(K, N, batch_size, epochs, max_steps)
    steps = ran * num_steps
    if steps == 0:
        return [epoch_means([], num_steps, ran) for _ in nets]
    X, x_stride = make_x(dev)
    Y = _f32(Y.reshape(N, -1), dev)
    pk = pack_members(nets, dev, one_kind=False)
    sizes, P, act = pk["sizes"], pk["P"], pk["act"]
    in_tr, out_tr = pk["tr"][:, :2 * sizes[0]].contiguous(), pk["tr"][:, 2 * sizes[0]:].contiguous()
    state = [opt._state(dev) for opt in opts]
    m, v = _stack([st[0] for st in state]), _stack([st[1] for st in state])      # (one member: the optimiser's own blocks)
    g = opts[0].param_groups[0]
    idx_d = torch.from_numpy(np.ascontiguousarray(idx)).to(dev)
    loss = torch.empty((K, steps), dtype=torch.float32, device=dev)
    net_args = (_ints(sizes), len(sizes), ptr(in_tr), ptr(out_tr))
    step_args = (ptr(idx_d), steps, int(batch_size), float(g['lr']), float(g['weight_decay']), ptr(loss))
    if entry == "mjx_dyn_fit_adam":
        check(load().mjx_dyn_fit_adam(ptr(X), ptr(Y), N, *net_args, target_mode, act, ptr(P), ptr(m), ptr(v), opts[0].step_count, *step_args,
                                      _stream(dev)))
    else:
        mode = () if entry == "mjx_reward_fit_ensemble" else (target_mode,)      # (the reward entry's target mode is its own)
        step0 = (ctypes.c_int64 * K)(*[int(opt.step_count) for opt in opts])
        route = ctypes.c_int(-1)
        check(getattr(load(), entry)(ptr(X), x_stride, ptr(Y), 0, N, K, *net_args, *mode, act, ptr(P), ptr(m), ptr(v), step0, *step_args,
                                     ctypes.byref(route), _stream(dev)))
    return _write_back(nets, opts, P, m, v, steps, loss.cpu().numpy(), num_steps, ran)


def _fit(net, opt, X, Y, target_mode, batch_size, epochs, max_steps):
    """one net through ``mjx_dyn_fit_adam`` (a one-member ensemble call runs another kernel and other bits)"""
    return _fit_members([net], [opt], lambda dev: (_f32(X, dev), 0), Y, target_mode, batch_size, epochs, max_steps, "mjx_dyn_fit_adam")[0]


def ensemble_fit_indices(K, num_samples, batch_size, epochs, max_steps=1e10):
    """the host side of K successive fits of one data set: member 0's permutations from NumPy's global stream, then member
    1's, ... exactly as K calls of :func:`fit_permutations` draw them (the early-stop message comes per member)
    -> (K x (steps * batch) int32 row indices, steps per epoch, epochs run)"""
    draws = [fit_permutations(num_samples, batch_size, epochs, max_steps) for _ in range(K)]
    if not draws:
        return np.zeros((0, 0), np.int32), int(num_samples // batch_size), 0
    return np.stack([d[0] for d in draws]), draws[0][1], draws[0][2]


def _same_fit(models):
    """may K WorldModels share one mjx_dyn_fit_ensemble call: one shape, activation, residual flag and optimiser setting"""
    n0, g0 = models[0].dynamics_net, models[0].dynamics_opt.param_groups[0]
    for mdl in models[1:]:
        n, g = mdl.dynamics_net, mdl.dynamics_opt.param_groups[0]
        if (tuple(n.layer_sizes) != tuple(n0.layer_sizes) or _act_code(n) != _act_code(n0) or bool(n.residual) != bool(n0.residual)
                or g['lr'] != g0['lr'] or g['weight_decay'] != g0['weight_decay']):
            return False
    return True


def fit_ensemble(models, s, a, sp, fit_mb_size, fit_epochs, max_steps=1e4, set_transformations=True, _draws=None):
    """``[mdl.fit_dynamics(s, a, sp, fit_mb_size, fit_epochs, max_steps, set_transformations) for mdl in models]`` (the
    driver's loop, run_model_accel_npg.py:168-177) with every member's Adam chain in ONE launch (``mjx_dyn_fit_ensemble``:
    a workgroup per member; shapes it does not serve run member by member inside the same call).  Per member the same
    transform expressions, the same draws from NumPy's global stream in the same order, the same optimiser state carried
    and advanced, the parameters written back and ``_generation`` bumped.  -> a list of K epoch-loss lists.  Members that
    differ in layer sizes, activation, ``residual`` or optimiser settings run the plain loop.  (_draws: the index draws made
    ahead by :func:`fit_world_models`.)"""
    models = list(models)
    if not models:
        return []
    if _draws is None and not _same_fit(models):
        return [mdl.fit_dynamics(s, a, sp, fit_mb_size, fit_epochs, max_steps=max_steps, set_transformations=set_transformations)
                for mdl in models]
    assert type(s) == type(a) == type(sp)
    assert s.shape[0] == a.shape[0] == sp.shape[0]
    if type(s) == np.ndarray:
        s = torch.from_numpy(s).float()
        a = torch.from_numpy(a).float()
        sp = torch.from_numpy(sp).float()
    nets, opts = [mdl.dynamics_net for mdl in models], [mdl.dynamics_opt for mdl in models]
    if set_transformations:
        for mdl, net in zip(models, nets):       # on each member's device, as fit_dynamics forms them
            net.set_transformations(*_dynamics_transforms(net.residual, s.to(mdl.device), a.to(mdl.device), sp.to(mdl.device)))
    return _fit_members(nets, opts, lambda dev: (_f32(torch.cat([s, a], -1), dev), 0), sp, TGT_RESIDUAL if nets[0].residual else TGT_PLAIN,
                        fit_mb_size, fit_epochs, max_steps, "mjx_dyn_fit_ensemble", _draws)


def _same_reward_fit(models):
    """:func:`_same_fit`'s rule for the reward nets: every member learns its reward, one shape, activation and optimiser setting"""
    if not all(mdl.learn_reward for mdl in models):
        return False
    n0, g0 = models[0].reward_net, models[0].reward_opt.param_groups[0]
    for mdl in models[1:]:
        n, g = mdl.reward_net, mdl.reward_opt.param_groups[0]
        if (tuple(n.layer_sizes) != tuple(n0.layer_sizes) or _act_code(n) != _act_code(n0) or g['lr'] != g0['lr']
                or g['weight_decay'] != g0['weight_decay']):
            return False
    return True


def fit_reward_ensemble(models, s, a, r, fit_mb_size, fit_epochs, max_steps=1e4, set_transformations=True, _draws=None):
    """``[mdl.fit_reward(s, a, r, fit_mb_size, fit_epochs, max_steps, set_transformations) for mdl in models]`` with every
    member's Adam chain in ONE launch (``mjx_reward_fit_ensemble``: a workgroup per member; shapes it does not serve run member by
    member inside the same call).  Per member the same transform expressions on the member's device, s' = the bits of
    ``mdl.dynamics_net.forward(s, a)`` (one :func:`ensemble_forward` over the K dynamics nets on the shared rows), the same draws
    from NumPy's global stream in member order, ``reward_opt`` carried and advanced, the parameters written back and
    ``_generation`` bumped.  -> a list of K epoch-loss lists.  Members that differ in layer sizes, activation or optimiser
    settings, or any member with ``learn_reward=False``, run the plain loop.  (_draws: as in :func:`fit_ensemble`.)"""
    models = list(models)
    if not models:
        return []
    if _draws is None and not _same_reward_fit(models):
        return [mdl.fit_reward(s, a, r, fit_mb_size, fit_epochs, max_steps=max_steps, set_transformations=set_transformations)
                for mdl in models]
    assert type(s) == type(a) == type(r)
    assert len(r.shape) == 2 and r.shape[1] == 1
    assert s.shape[0] == a.shape[0] == r.shape[0]
    if type(s) == np.ndarray:
        s = torch.from_numpy(s).float()
        a = torch.from_numpy(a).float()
        r = torch.from_numpy(r).float()
    if set_transformations:
        for mdl in models:                       # on each member's device, as fit_reward forms them
            mdl.reward_net.set_transformations(*_reward_transforms(s.to(mdl.device), a.to(mdl.device), r.to(mdl.device)))
    nets, opts = [mdl.reward_net for mdl in models], [mdl.reward_opt for mdl in models]

    def make_x(dev):
        sa = _f32(torch.cat([s, a], -1), dev)
        # s'_k = dynamics_net_k.forward(s, a): k_dyn_forward computes each row by itself, so the batched launch gives the same bits
        dyn = [mdl.dynamics_net for mdl in models]
        if len({tuple(d.layer_sizes) for d in dyn}) == 1:
            sp = ensemble_forward(dyn, sa, dev)
        else:
            sp = torch.stack([ensemble_forward([d], sa, dev)[0] for d in dyn])
        X = torch.cat([sa.unsqueeze(0).expand(len(models), -1, -1), sp], -1).contiguous()          # K x N x (2 n + m)
        return X, X.shape[1] * X.shape[2]

    return _fit_members(nets, opts, make_x, r, TGT_AFFINE, fit_mb_size, fit_epochs, max_steps, "mjx_reward_fit_ensemble", _draws)


def world_model_fit_indices(K, num_samples, batch_size, epochs, max_steps=1e10, learn_reward=True):
    """the host side of the driver's loop (run_model_accel_npg.py:170-178): member 0's dynamics permutations from NumPy's global
    stream, member 0's reward permutations, member 1's dynamics permutations, ... -> (dynamics draws, reward draws), each as
    :func:`ensemble_fit_indices` returns them; with learn_reward False: (``ensemble_fit_indices(...)``, None)"""
    if not learn_reward:
        return ensemble_fit_indices(K, num_samples, batch_size, epochs, max_steps), None
    dyn, rew = [], []
    for _ in range(K):
        dyn.append(fit_permutations(num_samples, batch_size, epochs, max_steps))
        rew.append(fit_permutations(num_samples, batch_size, epochs, max_steps))
    if not dyn:
        none = (np.zeros((0, 0), np.int32), int(num_samples // batch_size), 0)
        return none, none
    return tuple((np.stack([d[0] for d in draws]), draws[0][1], draws[0][2]) for draws in (dyn, rew))


def fit_world_models(models, s, a, sp, r, fit_mb_size, fit_epochs, max_steps=1e4, set_transformations=True):
    """the driver's fit loop (run_model_accel_npg.py:170-178, without the logging) --
    ``for mdl in models: mdl.fit_dynamics(s, a, sp, ...); mdl.fit_reward(s, a, r, ...)`` -- as two launches: all index draws
    first, in the driver's order (:func:`world_model_fit_indices`), then the dynamics ensemble fit, then the reward ensemble fit
    (it reads the fitted dynamics; stream order gives it that).  -> (K dynamics epoch-loss lists, K reward epoch-loss lists or
    None).  With no learned rewards it is :func:`fit_ensemble`; members that cannot share a call run the driver's loop."""
    models = list(models)
    if not models:
        return [], []
    if not any(mdl.learn_reward for mdl in models):
        return fit_ensemble(models, s, a, sp, fit_mb_size, fit_epochs, max_steps=max_steps, set_transformations=set_transformations), None
    if not (_same_fit(models) and _same_reward_fit(models)):
        dl, rl = [], []
        for mdl in models:
            dl.append(mdl.fit_dynamics(s, a, sp, fit_mb_size, fit_epochs, max_steps=max_steps, set_transformations=set_transformations))
            rl.append(mdl.fit_reward(s, a, r, fit_mb_size, fit_epochs, max_steps=max_steps, set_transformations=set_transformations)
                      if mdl.learn_reward else None)
        return dl, rl
    dyn_draws, rew_draws = world_model_fit_indices(len(models), int(sp.shape[0]), fit_mb_size, fit_epochs, max_steps, True)
    dl = fit_ensemble(models, s, a, sp, fit_mb_size, fit_epochs, max_steps=max_steps, set_transformations=set_transformations,
                      _draws=dyn_draws)
    rl = fit_reward_ensemble(models, s, a, r, fit_mb_size, fit_epochs, max_steps=max_steps, set_transformations=set_transformations,
                             _draws=rew_draws)
    return dl, rl


def ensemble_path_rewards(models, observations, actions):
    """``mdl.compute_path_rewards(dict(observations=observations[k], actions=actions[k]))`` for every member k: observations
    (K, N, H, n) and actions (K, N, H, m), as arrays or per-member lists -> rewards (K, N, H) float32.  One upload, one
    ``mjx_dyn_forward`` launch per (activation, flags) group over the K dynamics nets with per-member rows, one over the K
    reward nets, one read-back.  k_dyn_forward computes each row by itself: the result is the K single calls' bit for bit."""
    models = list(models)
    assert models and all(mdl.learn_reward for mdl in models), "every member must learn its reward"
    dev = _device()
    obs = np.ascontiguousarray(np.stack([np.asarray(o) for o in observations]) if isinstance(observations, (list, tuple)) else observations)
    act = np.ascontiguousarray(np.stack([np.asarray(o) for o in actions]) if isinstance(actions, (list, tuple)) else actions)
    K, N, H, n = obs.shape
    m = act.shape[-1]
    assert K == len(models) and act.shape[:3] == (K, N, H)
    if len({tuple(mdl.dynamics_net.layer_sizes) for mdl in models}) > 1 or len({tuple(mdl.reward_net.layer_sizes) for mdl in models}) > 1:
        out = []                                             # members of different shapes: one by one
        for k, mdl in enumerate(models):
            paths = dict(observations=obs[k], actions=act[k])
            mdl.compute_path_rewards(paths)
            out.append(paths['rewards'])
        return np.stack(out)
    # (compute_path_rewards: torch.from_numpy(s).float() on the host, then the copy)
    sa = np.concatenate([obs.reshape(K, N * H, n), act.reshape(K, N * H, m)], -1)
    sa = _f32(torch.from_numpy(sa).float(), dev)
    sp = ensemble_forward([mdl.dynamics_net for mdl in models], sa, dev)
    r = ensemble_forward([mdl.reward_net for mdl in models], torch.cat([sa, sp], -1), dev)
    return r.to('cpu').data.numpy().reshape(K, N, H)


def pack_dynamics_members(models, dev):
    """the device blocks a rollout over K members reads, for members that share shape, activation and flags (asserted):
    dict(sizes, P (K x params), tr (K x transforms), act, flags)"""
    return pack_members([mdl.dynamics_net for mdl in models], dev)


def pack_reward_members(models, dev):
    """the device blocks ``mjx_path_rewards`` reads, for K members that share shapes, activation and flags (asserted, as
    ``rollout_models`` does): dict(dyn_sizes, dyn_P, dyn_tr, dyn_act, dyn_flags, rew_sizes, rew_P, rew_tr, rew_act)"""
    models = list(models)
    assert models and all(mdl.learn_reward for mdl in models), "every member must learn its reward"
    dyn, rew = pack_members([mdl.dynamics_net for mdl in models], dev), pack_members([mdl.reward_net for mdl in models], dev)
    out = {"dyn_" + k: v for k, v in dyn.items()}
    out.update(("rew_" + k, v) for k, v in rew.items() if k != "flags")          # (a reward net's flags are OUT_AFFINE, always)
    return out


def cached_members_pack(stored, members, dev, with_rewards, extras=None):
    """THE device cache of ensemble members.  ``stored``: the (key, blocks, held) of an earlier call, or None -> (the tuple to store,
    whether the members were packed anew).  They are when :func:`members_pack_key` no longer gives the stored key: fresh blocks of
    :func:`pack_dynamics_members`, then ``extras(blocks)`` (a holder's own additions), then with ``with_rewards`` the blocks of
    :func:`pack_reward_members` under ``"rew"``."""
    key, held = members_pack_key(members, dev, with_rewards)
    if stored is not None and stored[0] == key:
        return stored, False
    pk = pack_dynamics_members(members, dev)
    if extras is not None:
        extras(pk)
    if with_rewards:
        pk["rew"] = pack_reward_members(members, dev)
    return (key, pk, held), True


def members_pack_key(members, dev, with_rewards):
    """What a device copy of ensemble members is made from -> (key, the tensors the key names).  Per member: the net's
    generation counter, which every write path of this package bumps (the fit's write-back through ``p.data.copy_``, which
    leaves ``p._version`` alone, ``set_params``, ``set_transformations``); per parameter and transform tensor its identity,
    ``_version`` (in-place edits) and storage; activation and flags.  With ``with_rewards`` the same for every member's reward
    net (``fit_reward``'s write-back bumps its counter), with output transforms that are plain numbers by value.  The tensors
    are returned to be HELD beside the key, so that an id() in it cannot come back as another tensor's."""
    nets = [mdl.dynamics_net for mdl in members]
    held = [t for net in nets for t in list(net.parameters()) + list(net.get_params()["transforms"])]
    if with_rewards:
        # the reward nets too; their out_shift / out_scale are plain numbers or tensors (nn_dynamics.py:281-311)
        rnets = [mdl.reward_net for mdl in members]
        nets = nets + rnets
        held += [t for net in rnets for t in list(net.parameters()) + list(net.get_params()["transforms"]) +
                 [v for v in (net.out_shift, net.out_scale) if isinstance(v, torch.Tensor)]]
        outs = tuple(float(v) for net in rnets for v in (net.out_shift, net.out_scale) if not isinstance(v, torch.Tensor))
    else:
        outs = ()
    key = (str(dev),) + outs + tuple((id(net), getattr(net, "_generation", 0), _act_code(net), _flags(net)) for net in nets) + \
        tuple((id(t), t._version, t.data_ptr()) for t in held)
    return key, held


def wide_rows_shape(dyn_sizes, rew_sizes=None):
    """whether the passes over stored rollouts hand a dynamics net (and a reward net, where one is given) to the ``_wide`` entries
    (``mjx_rollout_disagreement_wide``, ``mjx_path_rewards_wide``; csrc/rows_wide.h) when their caller asks for them: every net
    given with two hidden layers and a dynamics width above 128 -- wider than anything the register-resident routes take.  Plain
    Python, no library call; narrower on purpose than what the wide kernels serve (``mjx_..._wide_route``): the shapes that have
    a route today keep their call."""
    nets = [dyn_sizes] + ([] if rew_sizes is None else [rew_sizes])
    return all(len(sz) == 4 for sz in nets) and max(dyn_sizes[1:3]) > 128


def wide_entry(lib, name, wide):
    """``lib.mjx_<name>_wide`` where ``wide`` (the caller asked for it and its plain-Python shape predicate, :func:`wide_rows_shape`
    or ``sampling.wide_rollout_shape``, says so), else ``lib.mjx_<name>``: the same arguments either way"""
    return getattr(lib, "mjx_" + name + ("_wide" if wide else ""))


def predicted_route(lib, wide, switches, wide_query, narrow_query, *query_args):
    """the route an entry would report for these nets, before any call: 2 where ``wide`` (as :func:`wide_entry` takes it), every
    switch named in ``switches`` is on as the library reads it per call (on unless the variable starts with 0) and
    ``lib.<wide_query>`` answers 1; otherwise what ``lib.<narrow_query>`` answers (1: the register-resident MFMA kernel, 0: the
    generic route)"""
    if wide and all(os.environ.get(name, "1")[:1] != "0" for name in switches) and int(getattr(lib, wide_query)(*query_args)) == 1:
        return 2
    return int(getattr(lib, narrow_query)(*query_args))


def path_rewards_call(pk, obs_d, act_d, shared, rows, K, r32, r64, dev, wide=False):
    """one ``mjx_path_rewards`` over packed members (:func:`pack_reward_members`) -> the route taken.  ``wide``: where
    :func:`wide_rows_shape` says so, ``mjx_path_rewards_wide`` with the same arguments (route 2 = the wide MFMA kernel)"""
    route = ctypes.c_int(-1)
    m = pk["dyn_sizes"][0] - pk["dyn_sizes"][-1]
    lib = load()
    entry = wide_entry(lib, "path_rewards", wide and wide_rows_shape(pk["dyn_sizes"], pk["rew_sizes"]))
    check(entry(ptr(obs_d), ptr(act_d), 0 if shared else rows * m, rows, K, _ints(pk["dyn_sizes"]), len(pk["dyn_sizes"]),
                ptr(pk["dyn_P"]), ptr(pk["dyn_tr"]), pk["dyn_act"], pk["dyn_flags"], _ints(pk["rew_sizes"]),
                len(pk["rew_sizes"]), ptr(pk["rew_P"]), ptr(pk["rew_tr"]), pk["rew_act"],
                None if r32 is None else ptr(r32), None if r64 is None else ptr(r64), ctypes.byref(route), _stream(dev)))
    return route.value


def ensemble_path_rewards_device(models, obs_d, act_d, want64=False, packed=None, wide=False):
    """:func:`ensemble_path_rewards` on device data: obs_d (K, N, H, n) and act_d (K, N, H, m), or (N, H, m) shared by all members,
    fp32 device tensors -> rewards (K, N, H) fp32 on the device, with ``want64`` (fp32, the same values as fp64).  One
    ``mjx_path_rewards`` call (csrc/path_reward.h: both nets of a member in LDS on MFMAs where ``mjx_path_rewards_route`` says so,
    ``mjx_dyn_forward``'s kernel twice otherwise).  Members must share shapes, activation and flags.  The DATA make no host copy;
    the members' parameters and transforms are flattened and uploaded on every call unless ``packed`` carries the blocks of an
    earlier :func:`pack_reward_members` of the same, unchanged members on this device (``MPCPolicy`` keeps its own, keyed on the
    members' state).  ``wide``: as :func:`path_rewards_call`."""
    models = list(models)
    dev = obs_d.device
    assert obs_d.is_cuda and act_d.device == dev and obs_d.dtype == act_d.dtype == torch.float32, "fp32 device tensors"
    pk = packed if packed is not None else pack_reward_members(models, dev)
    assert pk["dyn_P"].device == dev and pk["dyn_P"].shape[0] == len(models), "packed blocks of these members on this device"
    K, N, H, n = obs_d.shape
    m = act_d.shape[-1]
    shared = act_d.dim() == 3
    assert K == len(models) and tuple(act_d.shape) == ((N, H, m) if shared else (K, N, H, m))
    assert (n + m, n) == (pk["dyn_sizes"][0], pk["dyn_sizes"][-1]), "the models' dims are not the data's"
    obs_d, act_d = obs_d.contiguous(), act_d.contiguous()
    r32 = torch.empty((K, N, H), dtype=torch.float32, device=dev)
    r64 = torch.empty((K, N, H), dtype=torch.float64, device=dev) if want64 else None
    path_rewards_call(pk, obs_d, act_d, shared, N * H, K, r32, r64, dev, wide=wide)
    return (r32, r64) if want64 else r32


def members_share_kind(models, with_rewards=False):
    """do the members share shape, activation and flags (what one launch over all of them needs; with ``with_rewards`` their reward
    nets too)?  What :func:`pack_members` asserts, as a question."""
    nets = [[mdl.dynamics_net for mdl in models]] + ([[mdl.reward_net for mdl in models]] if with_rewards else [])
    return all(len({(tuple(net.layer_sizes), _act_code(net), _flags(net)) for net in group}) == 1 for group in nets)


def rollout_disagreement_device(models, obs_d, act_d, packed=None, info=None, wide=False):
    """the ensemble-disagreement error (model_accel_npg.py:137-147) of rollouts that are on the device: obs_d (..., H, n) and act_d
    (..., H, m) fp32 device tensors, the stored rollouts of any number of paths (``train_step``: (K, N, H, .), all members' back to
    back) -> err (P, H - 1) fp32 on the device, err[p, t] = max over members of mean_c (obs[p, t + 1] - f_k(obs[p, t], act[p, t]))^2.
    One ``mjx_rollout_disagreement`` call (csrc/rollout_batch.h).  ``packed``: the blocks of :func:`pack_dynamics_members` (a
    :func:`cached_members_pack` holder's); ``info`` (a dict) receives ``route``.  ``wide``: where :func:`wide_rows_shape` says so,
    ``mjx_rollout_disagreement_wide`` with the same arguments (route 2 = the wide MFMA kernel, csrc/rows_wide.h)."""
    models = list(models)
    dev = obs_d.device
    assert obs_d.is_cuda and act_d.device == dev and obs_d.dtype == act_d.dtype == torch.float32, "fp32 device tensors"
    pk = packed if packed is not None else pack_dynamics_members(models, dev)
    sizes = tuple(pk["sizes"])
    n, m, H = obs_d.shape[-1], act_d.shape[-1], obs_d.shape[-2]
    assert (n + m, n) == (sizes[0], sizes[-1]) and pk["P"].shape[0] == len(models), "the models' dims are not the data's"
    assert obs_d.shape[:-1] == act_d.shape[:-1]
    obs_d, act_d = obs_d.contiguous(), act_d.contiguous()
    P = obs_d.numel() // (H * n) if H else 0
    err = torch.empty((P, max(H - 1, 0)), dtype=torch.float32, device=dev)
    route = ctypes.c_int(-1)
    lib = load()
    entry = wide_entry(lib, "rollout_disagreement", wide and wide_rows_shape(sizes))
    check(entry(ptr(obs_d), ptr(act_d), P, H, len(models), _ints(sizes), len(sizes), ptr(pk["P"]), ptr(pk["tr"]),
                pk["act"], pk["flags"], ptr(err), ctypes.byref(route), _stream(dev)))
    if info is not None:
        info["route"] = route.value
    return err


class DynamicsNet(nn.Module):
    def __init__(self, state_dim, act_dim, hidden_size=(64, 64),
                 s_shift=None,
                 s_scale=None,
                 a_shift=None,
                 a_scale=None,
                 out_shift=None,
                 out_scale=None,
                 out_dim=None,
                 residual=True,
                 seed=123,
                 use_mask=True,
                 ):
        """nn_dynamics.py:167-191: the same layers drawn from torch's stream after torch.manual_seed(seed)."""
        super(DynamicsNet, self).__init__()
        torch.manual_seed(seed)
        self.state_dim, self.act_dim, self.hidden_size = state_dim, act_dim, hidden_size
        self.out_dim = state_dim if out_dim is None else out_dim
        self.layer_sizes = (state_dim + act_dim, ) + tuple(hidden_size) + (self.out_dim, )
        self.fc_layers = nn.ModuleList([nn.Linear(self.layer_sizes[i], self.layer_sizes[i + 1])
                                        for i in range(len(self.layer_sizes) - 1)])
        self.nonlinearity = torch.relu
        self.residual, self.use_mask = residual, use_mask
        self._apply_out_transforms = True
        self._generation = 0        # bumped by every write of this package to the parameters or transforms (holders of device copies)
        self.set_transformations(s_shift, s_scale, a_shift, a_scale, out_shift, out_scale)

    def set_transformations(self, s_shift=None, s_scale=None,
                            a_shift=None, a_scale=None,
                            out_shift=None, out_scale=None):
        """nn_dynamics.py:193-228: tensors are kept as given, arrays become fp32 tensors, None = identity transforms"""
        given = (s_shift, s_scale, a_shift, a_scale, out_shift, out_scale)
        dims = (self.state_dim, self.state_dim, self.act_dim, self.act_dim, self.out_dim, self.out_dim)
        if s_shift is None:
            vals = [torch.full((k,), float(i % 2)) for i, k in enumerate(dims)]
        elif type(s_shift) in (torch.Tensor, np.ndarray):
            vals = [v if type(s_shift) == torch.Tensor else torch.from_numpy(np.float32(v)) for v in given]
        else:
            raise TypeError("Unknown type for transformations")
        device = next(self.parameters()).data.device
        (self.s_shift, self.s_scale, self.a_shift, self.a_scale, self.out_shift, self.out_scale) = [v.to(device) for v in vals]
        self.mask = self.out_scale >= 1e-8          # output columns without variation are forced to zero
        self._generation = getattr(self, "_generation", 0) + 1
        self.transformations = dict(s_shift=self.s_shift, s_scale=self.s_scale, a_shift=self.a_shift, a_scale=self.a_scale,
                                    out_shift=self.out_shift, out_scale=self.out_scale)

    def forward(self, s, a):
        """nn_dynamics.py:230-245 on the GPU (mjx_dyn_forward); returns a tensor on s's device (no autograd)"""
        if s.dim() != a.dim():
            print("State and action inputs should be of the same size")
        lead = s.shape[:-1]
        dev = _device()
        x = torch.cat([_f32(s, dev).reshape(-1, self.state_dim), _f32(a, dev).reshape(-1, self.act_dim)], -1)
        out = ensemble_forward([self], x, dev)[0]
        return out.reshape(*lead, self.out_dim).to(s.device)

    def get_params(self):
        network_weights = [p.data for p in self.parameters()]
        transforms = (self.s_shift, self.s_scale,
                      self.a_shift, self.a_scale,
                      self.out_shift, self.out_scale)
        return dict(weights=network_weights, transforms=transforms)

    def set_params(self, new_params):
        new_weights = new_params['weights']
        s_shift, s_scale, a_shift, a_scale, out_shift, out_scale = new_params['transforms']
        for idx, p in enumerate(self.parameters()):
            p.data = new_weights[idx]
        self._generation = getattr(self, "_generation", 0) + 1
        self.set_transformations(s_shift, s_scale, a_shift, a_scale, out_shift, out_scale)


class RewardNet(nn.Module):
    def __init__(self, state_dim, act_dim,
                 hidden_size=(64, 64),
                 s_shift=None,
                 s_scale=None,
                 a_shift=None,
                 a_scale=None,
                 seed=123,
                 ):
        """nn_dynamics.py:263-279: r = f(s, a, s')"""
        super(RewardNet, self).__init__()
        torch.manual_seed(seed)
        self.state_dim, self.act_dim, self.hidden_size = state_dim, act_dim, hidden_size
        self.layer_sizes = (state_dim + act_dim + state_dim, ) + tuple(hidden_size) + (1, )
        self.fc_layers = nn.ModuleList([nn.Linear(self.layer_sizes[i], self.layer_sizes[i + 1])
                                        for i in range(len(self.layer_sizes) - 1)])
        self.nonlinearity = torch.relu
        self.set_transformations(s_shift, s_scale, a_shift, a_scale)

    def set_transformations(self, s_shift=None, s_scale=None,
                            a_shift=None, a_scale=None,
                            out_shift=None, out_scale=None):
        """nn_dynamics.py:281-311: s' shares the s transforms; out_shift / out_scale are kept as given (0.0 / 1.0 if None)"""
        n, m = self.state_dim, self.act_dim
        if s_shift is None:
            vals = [torch.zeros(n), torch.ones(n), torch.zeros(m), torch.ones(m)]
            out_shift, out_scale = 0.0, 1.0
        elif type(s_shift) == torch.Tensor:
            vals = [s_shift, s_scale, a_shift, a_scale]
        elif type(s_shift) == np.ndarray:
            vals = [torch.from_numpy(v).float() for v in (s_shift, s_scale, a_shift, a_scale)]
        else:
            raise TypeError("Unknown type for transformations")
        device = next(self.parameters()).data.device
        self.s_shift, self.s_scale, self.a_shift, self.a_scale = [v.to(device) for v in vals]
        self.sp_shift, self.sp_scale = self.s_shift, self.s_scale
        self.out_shift, self.out_scale = out_shift, out_scale
        self.transformations = dict(s_shift=self.s_shift, s_scale=self.s_scale, a_shift=self.a_shift, a_scale=self.a_scale,
                                    out_shift=self.out_shift, out_scale=self.out_scale)

    def forward(self, s, a, sp):
        """nn_dynamics.py:313-328 on the GPU (mjx_dyn_forward)"""
        if s.dim() != a.dim():
            print("State and action inputs should be of the same size")
        lead = s.shape[:-1]
        dev = _device()
        n, m = self.state_dim, self.act_dim
        x = torch.cat([_f32(s, dev).reshape(-1, n), _f32(a, dev).reshape(-1, m), _f32(sp, dev).reshape(-1, n)], -1)
        return ensemble_forward([self], x, dev)[0].reshape(*lead, 1).to(s.device)

    def get_params(self):
        network_weights = [p.data for p in self.parameters()]
        transforms = (self.s_shift, self.s_scale,
                      self.a_shift, self.a_scale)
        return dict(weights=network_weights, transforms=transforms)

    def set_params(self, new_params):
        new_weights = new_params['weights']
        s_shift, s_scale, a_shift, a_scale = new_params['transforms']
        for idx, p in enumerate(self.parameters()):
            p.data = new_weights[idx]
        self.set_transformations(s_shift, s_scale, a_shift, a_scale)


def fit_model(nn_model, X, Y, optimizer, loss_func, batch_size, epochs, max_steps=1e10):
    """nn_dynamics.py:344-385 for this module's nets: X = (s, a) or (s, a, s'), Y the regression targets, optimizer a
    ``_DeviceAdam`` (a net's ``dynamics_opt`` / ``reward_opt``).  The loss is the MSE (loss_func is not called).  A
    DynamicsNet is fitted in the space it is in: with _apply_out_transforms False the targets are taken as given."""
    assert type(X) == tuple
    for d in X:
        assert type(d) == torch.Tensor
    assert type(Y) == torch.Tensor
    if isinstance(nn_model, RewardNet):
        mode = TGT_AFFINE
    elif nn_model._apply_out_transforms:
        raise MjxError("fit_model: a DynamicsNet is fitted with _apply_out_transforms = False (nn_dynamics.py:112)")
    else:
        mode = TGT_PLAIN
    if mode == TGT_PLAIN:          # Y is already the target: fit against identity output transforms
        saved = (nn_model.out_shift, nn_model.out_scale)
        nn_model.out_shift, nn_model.out_scale = torch.zeros(nn_model.out_dim), torch.full((nn_model.out_dim,), 1.0 - 1e-8)
        try:
            return _fit(nn_model, optimizer, torch.cat(X, -1), Y, mode, batch_size, epochs, max_steps)
        finally:
            nn_model.out_shift, nn_model.out_scale = saved
    return _fit(nn_model, optimizer, torch.cat(X, -1), Y, mode, batch_size, epochs, max_steps)
