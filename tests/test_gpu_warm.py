"""mpc_closed_loop_warm on the device: the traced loop with ws_carry_kernel building the solver's ubar of the listed
egos before the solve (the kept plan shifted by one stage, or the reference warm start restated) and ws_keep_kernel
keeping the solver's U by ego and accumulating the warm rows after the plant kernel (csrc/warm_kernels.h).  Every
comparison is bit for bit: mpc_closed_loop_traced for the reference warm start, with and without warm outputs, and a
sqp_iters = 0 solve for the warm start that is handed over; a stepwise restatement around
Solver.solve_batch(..., ubar=...) on the device that applies the carry rule in numpy; halves of the batch with
ego_offset.  The bodies are shared with tests/test_warm_cpu.py (warm_cases.py).  Trajectory1, N = 5 with 24 steps and
N = 20 with 30 steps, six egos."""
import pytest

import warm_cases as WC
import trace_cases as TRC

pytestmark = pytest.mark.gpu

CASES = [(N, noisy) for N in TRC.HORIZONS for noisy in (False, True)]
CARRIED = [(N, noisy, v) for N, noisy in CASES for v in WC.VARIANTS]


@pytest.fixture(scope="module")
def env():
    import __graft_entry__ as g
    g.build()
    import mpcqp
    import shard
    import trajectory_tracking as TT
    from trajectory_loader import TrajectoryLoader, builtin_trajectory
    traj = TrajectoryLoader(builtin_trajectory(1))
    solvers = {}

    def solver(N, max_obs=0, sqp_iters=1):
        key = (N, max_obs, sqp_iters)
        if key not in solvers:
            solvers[key] = mpcqp.Solver(traj.X_ref, traj.U_ref,
                                        mpcqp.default_params(N=N, max_obs=max_obs, sqp_iters=sqp_iters), device=0)
        return solvers[key]

    yield dict(mpcqp=mpcqp, shard=shard, TT=TT, traj=traj, solver=solver)
    for s in solvers.values():
        s.close()


@pytest.mark.parametrize("N,noisy", CASES)
def test_reference_with_nothing_requested_is_the_traced_entry(env, N, noisy):
    WC.check_anchor_off(env, N, noisy)


@pytest.mark.parametrize("N,noisy", CASES)
def test_materialised_reference_leaves_the_traced_outputs_alone(env, N, noisy):
    WC.check_anchor_on(env, N, noisy)


@pytest.mark.parametrize("N,noisy,variant", CARRIED)
def test_carried_loop_equals_the_restatement(env, N, noisy, variant):
    WC.check_restatement(env, N, noisy, variant)


@pytest.mark.parametrize("N,noisy,variant", CARRIED)
def test_known_answers(env, N, noisy, variant):
    WC.check_known_answers(env, N, noisy, variant)


@pytest.mark.parametrize("N,noisy,variant", [(5, True, "hold_nobs"), (20, False, "ref_tail")])
def test_composition_invariance(env, N, noisy, variant):
    WC.check_composition(env, N, noisy, variant)


def test_misuse(env):
    WC.check_misuse(env)
