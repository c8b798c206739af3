"""k_plan_rollout<HB, NB> and the four scoring kernels (csrc/plan.h) behind mjx_plan_rollout and mjx_plan_score per instance, width and
edge.  tests/test_gpu_mpc.py proves the shapes the planner needed; there h1 >= h2 in every case, at most two action slot groups
are live beside m = 28 and 32, the mask never sits in the second state block, flags 0 never runs, one scale serves all state columns,
nothing guards the output blocks and the scores give one number.  Here the inputs can tell those apart.  Cases, seeded recipes,
measures and check functions: tests/_plan_cases.py; every check runs in ONE fresh worker process under a time limit
(tests/_plan_matrix_worker.py; it took 0.7 s on the MI355X after the imports; the limit is 120 s); a worker that failed is not started
again -- the remaining tests fail with its output.  tests/test_plan_checks.py shows on the CPU that these checks pass NumPy
emulations of the kernels and flag the defects a wrong kernel would leave.

ROLLOUT.  Recipe: _mpc_learned_oracle.kernel_case's and _refine_oracle.kernel_case's nets and transforms; in every case one out_scale
entry is exactly 0 beside an out_shift of +-0.4, whatever the flags (column n // 2; column 36 on the n = 40 nets) -- but at n = 1 (r2,
h2), where the only column would be masked, every stored state would be s0 on both routes and nothing the kernel computes could show.
Axis cases: K = 2, H = 5, 165 rows (one workgroup plus a second with one full tile and one of five rows) and 6 rows, s0 as one state
(stride 0) and as (N, n), actions fp32 (N, H, m); all on route 1 by the host arithmetic (asserted on the CPU with mjx_plan_route):
    r1  (8, 8)    32 x 32 tanh    flags 3  <1,1>  no padding anywhere: n8 = n, m8 = m
    r2  (1, 1)    32 x 32 ReLU    flags 7  <1,1>  smallest everything (h2: the same nets at H = 1 -- only s0 is stored, exactly)
    r3  (11, 17)  32 x 64 ReLU    flags 5  <2,1>  h1 < h2: W2's row stride h1 under HB = 2; three action slot groups
    r4  (11, 25)  64 x 32 tanh    flags 1  <2,1>  four slot groups; h1 > h2
    r5  (32, 8)   96 x 96 tanh    flags 0  <3,1>  one state block exactly full; no output affine
    r6  (17, 6)   32 x 128 ReLU   flags 7  <4,1>  one layer-1 block under a four-block W2: the K dimension against the instance width
    r7  (33, 1)   32 x 32 ReLU    flags 7  <1,2>  one feature in the second state block; m = 1
    r8  (39, 28)  64 x 96 ReLU    flags 7  <3,2>  the Adroit dims; h1 < h2 on two state blocks
    r9  (64, 32)  128 x 128 ReLU  flags 7  <4,2>  the route's limits, the largest image (151.8 KiB)
    r10 (40, 5)   64 x 64 tanh    flags 3  <2,2>  the mask in the second state block; tanh on NB = 2
    f3, f9   r3's and r9's nets at H = 16, 33 rows: the free-running comparison over a long horizon
Geometry cases:
    g1  r3's shape, K = 5, N = 417, H = 3, per-trajectory s0: four workgroups per member, the last with a 32-row tile and a 1-row tile
        (two of its waves leave after the barrier); k * Pstride and the obs offset run past member 1
    g2  r7's shape, K = 1, N = 1, H = 1
    g3  r10's nets (NB = 2), H = 3, rows 31, 32, 33, 128, 129, s0 stride 0

Checks, on both routes (MJX_PLAN_MFMA 1 and 0) per run of a case: obs[:, :, 0] equals s0 bit for bit; every later stored state against
one fp64 step (_dyn_oracle.rollout_next) from the stored state and action before it, and against the free-running fp64 rollout
(_mpc_oracle.rollout); the routes against each other; the column with the zero out_scale exactly 0 (either sign) at t >= 1 under
flags 3 and exactly s0's column at every t under flags 7; different bits between the routes on every run of 32 rows or more (equal
bits would be a quiet fallback; the H = 1 cases store s0 alone and cannot differ).  The error is taken per state column of each
member, relative to that column's largest |reference| over the compared rows, and reported as the largest over columns, members and
runs (_plan_cases.col_err).  The zero-scale column is left out of the error where the mask flag is on (its reference is 0 or s0: it
is asserted exactly instead).  tests/test_plan_checks.py asserts from the oracle alone that every compared column reaches 1e-3 and no
state exceeds 1e3, so the measure never divides by noise.

Every obs block is prefilled with NaN and carries 64 NaN guard elements behind the last member's last row: no NaN may stay inside (a
tile that no wave owns) and no guard element may be touched (a store from a lane beyond N); the worker asserts both per call, as it
does for R, S and the sequence of every scoring call.  mjx_plan_rollout with s0_stride = n + 1, m = 0, a null s0, null actions or
K = 0 returns MJX_ERR_ARG and leaves a guarded output untouched.

Bars: the yardstick is the unmodified reference's own fp32 rollout (its DynamicsNet stepped by its trajectory_rollout) on the same
seeded inputs against the same fp64 oracle, measured in the same way on the CPU (tests/golden/make_golden_plan_matrix.py ->
tests/golden/plan_matrix.npz: "pstep_<case>" the per-column step error from the reference's own stored states, "pfree_<case>" the
free-running distance).  The bar is 3 x the yardstick for each route against fp64 (tests/test_gpu_path_rewards.py's MARGIN: two fp32
chains of equal length in different summation orders differ by a small multiple), and the sum of the two routes' free-running bars
between the routes (both lie within their bar of the same fp64 rollout).  No bar is a multiple of anything the kernels produced.
Measured on the MI355X [in brackets: route 1 / route 0 as a share of the bar]:
    f3   step: yardstick 5.895e-08  bar 1.769e-07  [0.35 / 0.32]   free: yardstick 1.847e-07  bar 5.540e-07  [0.33 / 0.33]   routes: bar 1.108e-06  [0.19]
    f9   step: yardstick 7.055e-08  bar 2.117e-07  [0.28 / 0.33]   free: yardstick 2.870e-07  bar 8.611e-07  [0.32 / 0.27]   routes: bar 1.722e-06  [0.16]
    g1   step: yardstick 5.933e-08  bar 1.780e-07  [0.33 / 0.33]   free: yardstick 8.857e-08  bar 2.657e-07  [0.33 / 0.33]   routes: bar 5.314e-07  [0.31]
    g3   step: yardstick 9.719e-07  bar 2.916e-06  [0.41 / 0.38]   free: yardstick 9.719e-07  bar 2.916e-06  [0.41 / 0.38]   routes: bar 5.831e-06  [0.20]
    r1   step: yardstick 2.861e-07  bar 8.584e-07  [0.43 / 0.31]   free: yardstick 2.848e-07  bar 8.544e-07  [0.43 / 0.30]   routes: bar 1.709e-06  [0.21]
    r2   step: yardstick 4.857e-08  bar 1.457e-07  [0.33 / 0.33]   free: yardstick 1.260e-07  bar 3.779e-07  [0.33 / 0.33]   routes: bar 7.557e-07  [0.18]
    r3   step: yardstick 1.509e-07  bar 4.528e-07  [0.36 / 0.33]   free: yardstick 2.492e-07  bar 7.477e-07  [0.35 / 0.33]   routes: bar 1.495e-06  [0.19]
    r4   step: yardstick 3.798e-07  bar 1.139e-06  [0.42 / 0.33]   free: yardstick 3.815e-07  bar 1.145e-06  [0.42 / 0.33]   routes: bar 2.289e-06  [0.17]
    r5   step: yardstick 1.058e-06  bar 3.175e-06  [0.33 / 0.38]   free: yardstick 1.058e-06  bar 3.175e-06  [0.35 / 0.38]   routes: bar 6.350e-06  [0.21]
    r6   step: yardstick 2.491e-07  bar 7.474e-07  [0.37 / 0.33]   free: yardstick 3.217e-07  bar 9.651e-07  [0.41 / 0.39]   routes: bar 1.930e-06  [0.17]
    r7   step: yardstick 3.425e-07  bar 1.028e-06  [0.29 / 0.30]   free: yardstick 6.585e-07  bar 1.975e-06  [0.28 / 0.32]   routes: bar 3.951e-06  [0.16]
    r8   step: yardstick 1.875e-07  bar 5.624e-07  [0.36 / 0.32]   free: yardstick 3.109e-07  bar 9.326e-07  [0.38 / 0.29]   routes: bar 1.865e-06  [0.20]
    r9   step: yardstick 3.232e-07  bar 9.696e-07  [0.42 / 0.30]   free: yardstick 4.275e-07  bar 1.283e-06  [0.45 / 0.33]   routes: bar 2.565e-06  [0.25]
    r10  step: yardstick 7.685e-07  bar 2.305e-06  [0.41 / 0.27]   free: yardstick 7.672e-07  bar 2.302e-06  [0.41 / 0.27]   routes: bar 4.603e-06  [0.19]

SCORING (mjx_plan_score: obs fp32, rewards and actions fp64; the reference's index, the per-trajectory index and obs = None).  Shapes
(K, N, H, n, m), kappa 3, gamma 0.95, omega 2 unless named:
    t1023 (3, 341, 4, 3, 2)  t1024 (4, 256, 4, 3, 2)  t1025 (5, 205, 4, 3, 2)   T = K N around k_plan_softmax's 1024 threads
    n255 (2, 255, 4, 3, 2)   n257 (2, 257, 4, 3, 2)   [t1024 has N = 256]        N around k_plan_sequence's stride of 256
    hn63 (3, 40, 9, 7, 2)    hn64 (3, 40, 8, 8, 2)    hn65 (3, 40, 13, 5, 2)     H n around k_plan_disagree's wave stride of 64
    k1 (1, 40, 6, 5, 3): every std is exactly 0, so R with obs given equals R without, bit for bit;  one (1, 1, 1, 1, 1);
    h1 (3, 40, 1, 5, 3);  wide (2, 2, 3, 65, 33) with kappa 0.5, gamma 0.99, omega 1, from tests/test_gpu_mpc.py
on (4, 300, 6, 5, 3):
    gam0 (gamma 0: 0^0 = 1), gam1, gamh (0.5);  om0 (omega 0 with obs given);  kap0 (all S = 1 exactly);
    kap800 (rewards x 10, the scores spread over more than 5 units: most S underflow to exactly 0, the sequence must still match);
    equal (all rewards equal: without obs every R is equal and every S is 1);
    max0, maxT: the unique maximum (reward + 50) planted at element 0 and at T - 1; maxw15: at element 1024 + 1000, whose tid 1000 lies
    in wave 15 on the second stride pass -- that needs T > 2024, so this case alone has N = 600
In every case the device's largest score has the weight exactly 1, and in the planted cases it is the planted element and no other.
Argument checks: K = 0, K = 65536, N = 0, idx_mode 2 and the reference index with K = 4 > N = 3 and obs given each return MJX_ERR_ARG
with the guarded R, S and sequence untouched.

Bounds.  The reference of every measure is the reference's expressions in np.longdouble (_plan_cases.score_ld, 64 mantissa bits,
asserted); R, S and the sequence are measured each on its own, per element, against a forward bound of the kernel's fixed summation
order (_plan_cases.score_bounds), u = 2^-53, g(k) = k u / (1 - k u); the bar is 1.
  disagreement (k_plan_disagree), per element e of the H n: the fp32 inputs widen exactly; the mean is K - 1 sums and a division,
    |dmean| <= g(K) mean|a|; d_k = a_k - mean rounds once and carries the mean's error, e_d = u |d_k| + |dmean|; the sum of squares
    takes (2 |d_k| + e_d) e_d from its inputs and g(K + 1) of itself from K products and K sums; the division by K one more u; the
    root |sqrt(v +- e) - sqrt(v)| <= min(e / sqrt(v), sqrt(e)) and the device's sqrt.  With K = 1 every term is 0: the bound asks for
    an exact 0.  A lane sums ceil(H n / 64) values in index order and the wave adds six xor levels: g(ceil(H n / 64) + 6) of sum std.
  R (k_plan_returns): B_R = |omega| B_dis + g(H + U_pow + 2) (|omega| dis + sum_t gamma^t |r_t|) -- omega dis rounds once; each term
    has pow, one product and at most H sums.
  S (k_plan_softmax): the device's maximum lies within B_mx = the largest B_R among the scores that can reach the top; the argument
    kappa (R - max) carries |kappa| (B_R + B_mx) and two roundings of itself, dx; B_S = S (expm1(dx) (1 + g(U_exp)) + g(U_exp)) +
    (U_exp + 1) 2^-1074 (the last term where S is subnormal or underflows: the long-double reference does not).
  sequence (k_plan_sequence): the numerator is a sum over N of (sum over K members of S) a: g(K + 1 + ceil(N / 256) + 6 + 3) of
    sum_i w_i |a_ie| plus sum_i B_w |a_ie|; sum S is a strided sum of ceil(T / 1024), six xor levels and sixteen waves in order; the
    denominator sum S + 1e-6 rounds once; the quotient once.
U_exp = U_pow = U_sqrt = 2 ulp.  This is an ASSUMPTION: ROCm's table of its device math functions' accuracy is not among the files of the
ROCm installation the suite was written on, so 2 ulp each stands in for it.
NumPy's own fp64 evaluation of the reference's lines (_mpc_oracle.scores / weights / sequence) stays inside the same bounds on every
case (tests/test_plan_checks.py).  Measured on the MI355X, the largest share of each bound [R / S / sequence]:
    t1023 0.243 / 0.202 / 0.010;  t1024 0.209 / 0.212 / 0.007;  t1025 0.262 / 0.156 / 0.012;  n255 0.235 / 0.191 / 0.008
    n257 0.210 / 0.155 / 0.008;  hn63 0.136 / 0.109 / 0.013;  hn64 0.115 / 0.121 / 0.015;  hn65 0.111 / 0.065 / 0.012
    k1 0.156 / 0.122 / 0.017;  one 0.000 / 0.000 / 0.015;  h1 0.095 / 0.212 / 0.015;  wide 0.062 / 0.161 / 0.038
    gam0 0.064 / 0.142 / 0.005;  gam1 0.236 / 0.151 / 0.019;  gamh 0.292 / 0.303 / 0.009;  om0 0.197 / 0.140 / 0.005
    kap0 0.193 / 0.000 / 0.011;  kap800 0.210 / 0.027 / 0.000;  equal 0.084 / 0.032 / 0.004;  max0 0.230 / 0.158 / 0.000
    maxT 0.167 / 0.125 / 0.000;  maxw15 0.201 / 0.177 / 0.000
[no unwritten element and no touched guard element in 306 guarded blocks: 108 rollout calls and 66 scoring calls with three blocks
each; every argument check returned MJX_ERR_ARG and wrote nothing; every case is served by route 1 and the routes' bits differ on every
run of 32 rows or more.  No defect found.]"""
import os
import sys

import pytest

from tests._worker_run import worker_result

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _plan_cases as C  # noqa: E402

LIMIT = 120

pytestmark = pytest.mark.gpu


def _result():
    return worker_result("_plan_matrix_worker.py", LIMIT, "plan matrix")


def _checks(case):
    rec = _result()["rollout"][case]
    ps, pf = C.yard(case) if case in C.STEPPED else (None, None)
    if ps is not None:
        bs, bf = C.MARGIN * ps, C.MARGIN * pf
        print(case, "yardsticks %.3e %.3e bars %.3e %.3e; shares: step %.2f / %.2f, free %.2f / %.2f, routes %.2f"
              % (ps, pf, bs, bf, rec["step"]["1"] / bs, rec["step"]["0"] / bs, rec["free"]["1"] / bf, rec["free"]["0"] / bf, rec["routes"] / (2 * bf)))
    return C.checks(case, rec, ps, pf), rec


def test_the_worker_ran_once_and_took_a_few_seconds():
    r = _result()
    print("worker: %.1f s, %d guarded blocks" % (r["seconds"], r["guarded_calls"]))
    assert r["seconds"] < 60.0


@pytest.mark.parametrize("case", C.STEPPED)
def test_route_1_against_fp64_per_column(case):
    ok, rec = _checks(case)
    ps, pf = C.yard(case)
    assert rec["step"]["1"] < C.MARGIN * ps and rec["free"]["1"] < C.MARGIN * pf and ok["mfma"]


@pytest.mark.parametrize("case", C.STEPPED)
def test_route_0_against_fp64_per_column(case):
    """MJX_PLAN_MFMA=0: k_model_rollout with the actions given (and k_plan_tile_s0 where s0 is one state)"""
    ok, rec = _checks(case)
    ps, pf = C.yard(case)
    assert rec["step"]["0"] < C.MARGIN * ps and rec["free"]["0"] < C.MARGIN * pf and ok["generic"]


@pytest.mark.parametrize("case", C.STEPPED)
def test_routes_agree(case):
    ok, rec = _checks(case)
    assert rec["routes"] < 2 * C.MARGIN * C.yard(case)[1] and ok["routes"]


@pytest.mark.parametrize("case", C.ORDER)
def test_first_stored_state_is_s0_and_the_zero_scale_column_is_exact(case):
    ok, rec = _checks(case)
    assert rec["s0_exact"] is True and rec["masked_exact"] is True and ok["s0"] and ok["masked"]


@pytest.mark.parametrize("case", C.ORDER)
def test_every_state_is_written_and_no_guard_element(case):
    ok, rec = _checks(case)
    assert rec["unwritten"] == 0 and rec["guard"] == 0 and ok["written"]
    assert rec["calls"] == 2 * len(C.CASES[case]["rows"]) * len(C.CASES[case]["s0"])


@pytest.mark.parametrize("case", C.ORDER)
def test_route_1_really_runs_its_own_kernel(case):
    """mjx_plan_route promises route 1 for every case; equal bits between the routes on a run of 32 rows or more would be a quiet
    fallback to k_model_rollout (H = 1 stores s0 alone: nothing to differ)"""
    ok, rec = _checks(case)
    assert _result()["served"][case] == 1
    assert rec["same_bits"] == [] and ok.get("own_kernel", True)


def test_rollout_argument_checks_return_err_arg_and_write_nothing():
    r = _result()
    print(r["rollout_args"])
    assert set(r["rollout_args"]) == {"s0_stride", "m_zero", "null_s0", "null_actions", "K_zero"}
    assert all(v == r["err_arg"] == -1 for v in r["rollout_args"].values())
    assert r["rollout_args_untouched"] is True


@pytest.mark.parametrize("case", C.SCORE_ORDER)
def test_scores_weights_and_sequence_each_inside_its_bound(case):
    rec = _result()["score"][case]
    print(case, "shares of the bounds: R %.3f S %.3f seq %.3f" % (rec["R"], rec["S"], rec["seq"]), rec)
    ok = C.score_checks(rec)
    assert rec["R"] <= 1.0 and rec["S"] <= 1.0 and rec["seq"] <= 1.0 and ok["R"] and ok["S"] and ok["seq"]
    assert rec["calls"] == len(C.score_modes(case)) == 3


@pytest.mark.parametrize("case", C.SCORE_ORDER)
def test_score_blocks_are_written_and_what_the_case_is_here_for_holds(case):
    """no NaN inside R, S or the sequence and no guard element touched; the device's maximum has the weight exactly 1; K = 1 adds an
    exact 0, kappa 0 gives S = 1, equal rewards equal R, kappa 800 underflows most S to 0, a planted maximum is found where it is"""
    ok = C.score_checks(_result()["score"][case])
    assert ok["written"] and ok["max_weight_one"] and ok["special"]


def test_score_argument_checks_return_err_arg_and_write_nothing():
    r = _result()
    print(r["score_args"])
    assert set(r["score_args"]) == {"K_zero", "K_65536", "N_zero", "idx_mode_2", "reference_K_gt_N"}
    assert all(v == r["err_arg"] == -1 for v in r["score_args"].values())
    assert r["score_args_untouched"] is True
