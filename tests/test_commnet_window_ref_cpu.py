"""CPU: the float64 reference of the non-recurrent CommNet module's window backward (tests/commnet_window_ref.py) against torch
float64 autograd through a transcription of the module's generic forward (ic3net_amd/comm.py forward(), the non-recurrent
branch: encoder -> tanh -> per pass the dense N x N masked communication, C_i, f_i, tanh -> heads) — the reference the host-build
and GPU tests of ic3_commnet_backward stand on.  Bar: 1e-10 relative, float64 against float64."""
import numpy as np
import pytest
import torch

import commnet_window_ref as ref

BAR = 1e-10


def _comm_dense(h, alive, gate, mode_avg, comm_zero):
    """comm.py:168-205 as the reference writes it: h (E, N, H) -> comm_sum (E, N, H) through the (E, N, N, H) tensor"""
    E, N, H = h.shape
    agent_mask = alive.view(E, 1, N).expand(E, N, N).unsqueeze(-1).clone()            # [e, i, j] = alive[j]
    num_alive = alive.sum(1)
    agent_mask = agent_mask * gate.view(E, 1, N).expand(E, N, N).unsqueeze(-1)
    agent_mask_t = agent_mask.transpose(1, 2)
    comm = h.unsqueeze(2).expand(E, N, N, H)                                          # [e, i, j, :] = h[e, i, :]
    mask = torch.zeros(N, N, dtype=h.dtype) if comm_zero else torch.ones(N, N, dtype=h.dtype) - torch.eye(N, dtype=h.dtype)
    comm = comm * mask.view(1, N, N, 1)
    if mode_avg:
        scale = torch.where(num_alive > 1, 1.0 / (num_alive - 1).clamp(min=1), torch.ones_like(num_alive))
        comm = comm * scale.view(E, 1, 1, 1)
    comm = comm * agent_mask * agent_mask_t
    return comm.sum(1)


CASES = [
    # P, mode_avg, hard attention gates, comm_mask_zero, share_weights
    (1, True, False, False, False),
    (2, True, True, False, False),
    (3, False, True, False, False),
    (2, False, False, False, True),
    (3, True, True, True, False),
    (2, True, True, False, True),
]


@pytest.mark.parametrize("P,mode_avg,hard,comm_zero,share", CASES)
def test_reference_against_autograd(P, mode_avg, hard, comm_zero, share):
    T, E, N, H, OT, obs_dim = 3, 4, 5, 8, 6, 11
    rng = np.random.default_rng(100 * P + 10 * mode_avg + hard)
    w = ref.make_weights(7 + P, H, P, OT, obs_dim, share=share)
    alive, gate = ref.make_masks(rng, T, E, N, dead=0.25, gated=0.4 if hard else 0.0)
    obs = rng.standard_normal((T, E * N, obs_dim))
    dhead = rng.standard_normal((T, E * N, OT))
    want = ref.reference_of(w, obs, dhead, E, N, alive=alive, gate=gate if hard else None, mode_avg=mode_avg, comm_zero=comm_zero)

    t64 = lambda a: torch.tensor(np.asarray(a, np.float64), requires_grad=True)
    wt, eb, wh = t64(w['enc_wt']), t64(w['enc_bias']), t64(w['w_heads'])
    nmod = 1 if share else P
    Fw, Cw, bs = [t64(w['f_w'][i]) for i in range(nmod)], [t64(w['c_w'][i]) for i in range(nmod)], [t64(w['bias'][i]) for i in range(nmod)]
    pick = lambda lst, i: lst[0] if share else lst[i]
    hb = torch.zeros(OT, dtype=torch.float64, requires_grad=True)
    loss = 0.0
    for t in range(T):
        x = torch.tanh(torch.tensor(obs[t]) @ wt + eb)
        h = x
        al = torch.tensor(alive[t], dtype=torch.float64)
        gt = torch.tensor(gate[t], dtype=torch.float64) if hard else torch.ones(E, N, dtype=torch.float64)
        for i in range(P):
            comm = _comm_dense(h.view(E, N, H), al, gt, mode_avg, comm_zero).reshape(E * N, H)
            h = torch.tanh(x + h @ pick(Fw, i).t() + comm @ pick(Cw, i).t() + pick(bs, i))
            assert np.abs(h.detach().numpy() - want['h_pass'][i + 1, t]).max() <= BAR
        loss = loss + ((h @ wh.t() + hb) * torch.tensor(dhead[t])).sum()
    loss.backward()

    def close(got, exp, what):
        err = np.abs(got.numpy() - exp).max() / max(1.0, np.abs(exp).max())
        assert err <= BAR, (what, err)
    close(wt.grad, want['enc_dwt'], 'encoder weight')
    close(eb.grad, want['enc_db'], 'encoder bias')
    close(wh.grad, want['heads_w'], 'heads weight')
    close(hb.grad, want['heads_b'], 'heads bias')
    for i in range(nmod):
        over = range(P) if share else (i,)
        close(Fw[i].grad, sum(want['f_grad'][j] for j in over), 'F %d' % i)
        close(Cw[i].grad, sum(want['c_grad'][j] for j in over), 'C %d' % i)
        close(bs[i].grad, sum(want['bias_cols'][j] for j in over), 'bias %d' % i)
    if comm_zero:
        assert all(np.abs(g).max() == 0.0 for g in want['c_grad'])


def test_reference_pieces_are_consistent():
    """de and dz as the reference returns them: de = (sum_i dz_i + dh0)(1 - h_0^2), and one step alone equals the window of it."""
    T, E, N, H, OT, obs_dim, P = 2, 3, 4, 8, 5, 9, 2
    rng = np.random.default_rng(5)
    w = ref.make_weights(3, H, P, OT, obs_dim)
    alive, gate = ref.make_masks(rng, T, E, N, dead=0.2, gated=0.3)
    obs, dhead = rng.standard_normal((T, E * N, obs_dim)), rng.standard_normal((T, E * N, OT))
    both = ref.reference_of(w, obs, dhead, E, N, alive=alive, gate=gate)
    assert np.allclose(both['de'], (both['dz'].sum(0) + both['dh0']) * (1 - both['h_pass'][0] ** 2), rtol=0, atol=1e-14)
    one = [ref.reference_of(w, obs[t:t + 1], dhead[t:t + 1], E, N, alive=alive[t:t + 1], gate=gate[t:t + 1]) for t in range(T)]
    for k in ('f_grad', 'c_grad', 'bias_cols'):
        for i in range(P):
            assert np.allclose(both[k][i], one[0][k][i] + one[1][k][i], rtol=0, atol=1e-12)
    assert np.allclose(both['enc_dwt'], one[0]['enc_dwt'] + one[1]['enc_dwt'], rtol=0, atol=1e-12)
