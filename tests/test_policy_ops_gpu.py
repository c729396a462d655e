"""GPU: the launch-chain kernels of csrc/policy_ops.hip through the ops.* wrappers (lstm_cell_, lstm_cell_backward, policy_heads,
lstm_cell_heads_, comm_masked_mean_raw, sample_actions[_env]) against the float64 references of tests/policy_ops_ref.py, on every
branch: all seven H/4 instances of the cell backward with dc absent / separate / aliased, bias partials row by row, the grid-stride
loop; the three NMAX instances and the scalar fallback of the communication block with its addend / row_scale / strided forms; both
column instances of the fused cell + heads kernel; sampling from a column slice.  The twin of tests/test_host_policy_ops_cpu.py: the
cases and assertions are policy_ops_ref.run_*, the bar keys carry the gpu/ prefix."""
import numpy as np
import pytest
import torch

import policy_ops_ref as ref

pytestmark = pytest.mark.gpu

PREFIX = 'gpu/'
NAN = float('nan')


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return None if t is None else t.cpu().numpy()


class GpuBackend(object):
    def cell_backward(self, gates, c_prev, dh, dc, alias, parts):
        from ic3net_amd import ops
        R, H = c_prev.shape
        dg = torch.full((R, 4 * H), NAN, device='cuda')
        dc_t = dev(dc)
        dcp = dc_t if alias else torch.full((R, H), NAN, device='cuda')
        pr = torch.full((ops.LSTM_BWD_MAX_PARTIALS, 4 * H), NAN, device='cuda') if parts else None
        view = ops.lstm_cell_backward(dev(gates), dev(c_prev), dev(dh), dc_t, dg, dcp, pr)
        return (view.shape[0] if parts else None), host(dg), host(dcp), host(pr)      # (the wrapper tells the count by its view)

    def cell_forward(self, gates, c, H):
        from ic3net_amd import ops
        c1 = dev(c)
        xh = torch.full((c.shape[0], 2 * H + ref.PAD), NAN, device='cuda')
        ops.lstm_cell_(dev(gates), c1, xh[:, H + ref.PAD:])
        return host(c1), host(xh)

    def heads(self, xh, H, W, b, sizes):
        from ic3net_amd import ops
        out = torch.full((xh.shape[0], W.shape[0]), NAN, device='cuda')
        return host(ops.policy_heads(dev(xh)[:, H + ref.PAD:], dev(W), dev(b), sizes, out=out))

    def cell_heads(self, gates, c, H, W, b, sizes, env):
        from ic3net_amd import ops
        R = c.shape[0]
        c1 = dev(c)
        xh = torch.full((R, 2 * H + ref.PAD), NAN, device='cuda')
        out = torch.full((R, W.shape[0]), NAN, device='cuda')
        act = torch.full((len(sizes), env.nenvs, R // env.nenvs), -1, dtype=torch.int32, device='cuda') if env is not None else None
        ops.lstm_cell_heads_(dev(gates), c1, xh[:, H + ref.PAD:], dev(W), dev(b), sizes, out=out, env=env, action=act)
        return host(c1), host(xh), host(out), host(act)

    def comm(self, h, H, alive, gate, avg, mask_self, addend, add_col0, row_scale):
        from ic3net_amd import ops
        E, N, _ = h.shape
        out = torch.full((E, N, H), NAN, device='cuda')
        add = dev(addend)[:, :, add_col0:add_col0 + H] if addend is not None else None
        ops.comm_masked_mean_raw(dev(h)[:, :, :H], dev(alive), dev(gate), avg, mask_self, out=out, addend=add,
                                 row_scale=dev(None if row_scale is None else row_scale.reshape(-1)))
        return host(out)

    def sample(self, wide, col0, A, head, seed, offset, episode, t):
        from ic3net_amd import ops
        act, chosen = ops.sample_actions(dev(wide)[:, :, col0:col0 + A], head, seed, offset, episode, t, want_logp=True)
        return host(act), host(chosen)

    def sample_env(self, env, wide, col0, A, head):
        from ic3net_amd import ops
        return host(ops.sample_actions_env(env, dev(wide)[:, :, col0:col0 + A], head))

    def make_env(self, E, N):
        from test_env_parity_gpu import make_pp
        env = make_pp(N, 8, 1, "mixed", E, seed=9, offset=4)
        env.reset()
        rng = np.random.default_rng(E + N)
        for _ in range(3):                                  # move the device-side (episode, t) counters off zero
            env.step(dev(rng.integers(0, 5, (E, N)).astype(np.int32)))
        return env

    def env_counters(self, env):
        st = env.get_state()
        return 9, 4, np.asarray(st['episode']).reshape(-1), np.asarray(st['t']).reshape(-1)

    def refusal(self, which):
        from ic3net_amd import ops
        H, sizes = ref.refusal_args(which)
        R, OT = 3, sum(sizes) + 1
        z = lambda *s: np.zeros(s, np.float32)
        if which.startswith('cell_backward'):
            ops.lstm_cell_backward(dev(z(R, 4 * H)), dev(z(R, H)), dev(z(R, H)), None, dev(z(R, 4 * H)), dev(z(R, H)), None)
        elif which.startswith('cell_heads'):
            self.cell_heads(z(R, 4 * H), z(R, H), H, z(OT, H), z(OT), sizes, None)
        else:
            self.heads(z(R, 2 * H + ref.PAD), H, z(OT, H), z(OT), sizes)


@pytest.fixture(scope="module")
def be():
    return GpuBackend()


@pytest.mark.parametrize("case", ref.cell_backward_cases(), ids=ref.cell_backward_id)
def test_cell_backward_against_float64(be, case):
    ref.run_cell_backward(be, PREFIX, *case)


@pytest.mark.parametrize("H", ref.CELL_FWD_H)
def test_cell_forward_against_float64(be, H):
    ref.run_cell_forward(be, PREFIX, H)


@pytest.mark.parametrize("H", ref.HEADS_H)
def test_policy_heads_against_float64(be, H):
    ref.run_heads(be, PREFIX, H)


@pytest.mark.parametrize("H", ref.FUSED_H)
def test_fused_cell_heads_against_float64_and_the_oracle_draw(be, H):
    ref.run_fused(be, PREFIX, H)


@pytest.mark.parametrize("case", ref.comm_cases(), ids=ref.comm_id)
def test_comm_block_against_the_literal_form(be, case):
    ref.run_comm(be, PREFIX, case)


@pytest.mark.parametrize("E,N", ref.SAMPLE_EN)
@pytest.mark.parametrize("A", ref.SAMPLE_A)
def test_sample_actions_against_the_oracle_draw(be, A, E, N):
    ref.run_sample(be, A, E, N)


def test_sample_actions_never_draws_a_zero_probability(be):
    ref.run_sample(be, 5, 51, 5, zero_prob=True)


@pytest.mark.parametrize("which", sorted(ref.REFUSALS))
def test_refusals_are_argument_checks(be, which):
    ref.run_refusal(be, which)
    torch.cuda.synchronize()                                # nothing was launched: nothing can have gone wrong on the device
