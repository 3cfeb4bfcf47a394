"""mpc_closed_loop_traced on the device: the noisy loop with the solver's U and Xpred of every step kept for the
listed egos, tg_gap_kernel accumulating the plan-vs-outcome gaps of every ego after the plant kernel and
tg_hist_kernel scattering the plans of the named egos (csrc/trace_kernels.h).  Every comparison is bit for bit:
mpc_closed_loop_noisy for everything the noisy entry has, with and without trace outputs; a stepwise restatement
around Solver.solve_batch on the device that keeps each step's U and Xpred, with the gap columns computed from them
in numpy; halves of the batch with ego_offset.  The bodies are shared with tests/test_trace_cpu.py
(trace_cases.py).  Trajectory1, N = 5 with 24 steps and N = 20 with 30 steps, six egos."""
import pytest

import trace_cases as TRC

pytestmark = pytest.mark.gpu

CASES = [(N, noisy) for N in TRC.HORIZONS for noisy in (False, True)]


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

    def solver(N, max_obs=0):
        if (N, max_obs) not in solvers:
            solvers[N, max_obs] = mpcqp.Solver(traj.X_ref, traj.U_ref, mpcqp.default_params(N=N, max_obs=max_obs),
                                               device=0)
        return solvers[N, max_obs]

    yield dict(mpcqp=mpcqp, shard=shard, TT=TT, traj=traj, solver=solver)
    for s in solvers.values():
        s.close()


@pytest.mark.parametrize("N,noisy", CASES)
def test_nothing_requested_is_the_noisy_entry(env, N, noisy):
    TRC.check_anchor_off(env, N, noisy)


@pytest.mark.parametrize("N,noisy", CASES)
def test_traces_leave_the_noisy_outputs_alone(env, N, noisy):
    TRC.check_anchor_on(env, N, noisy)


@pytest.mark.parametrize("N,noisy", CASES)
def test_traces_equal_the_restatement(env, N, noisy):
    TRC.check_restatement(env, N, noisy)


@pytest.mark.parametrize("N,noisy", CASES)
def test_known_answers(env, N, noisy):
    TRC.check_known_answers(env, N, noisy)


@pytest.mark.parametrize("N,noisy", [(5, True), (20, False)])
def test_composition_invariance(env, N, noisy):
    TRC.check_composition(env, N, noisy)


def test_misuse(env):
    TRC.check_misuse(env)
