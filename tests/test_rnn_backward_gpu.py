"""GPU: the tanh-recurrence baseline's window backward (ic3_rnn_backward, bptt._backward_window_rnn) — its two kernels against
float64, run-to-run identity, whole updates against the per-step loop (bptt._backward_episode_baseline) on the same record and
against autograd through the rollout replaying the same actions, the benchmark geometry, and which path each policy takes."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _rn(gen, *s):
    return torch.randn(*s, device='cuda', generator=gen, dtype=torch.float64)


@pytest.mark.parametrize("H,R,OT", [(64, 333, 6), (128, 64 * 70 + 17, 16), (128, 81920, 6)])
def test_tanh_step_against_float64(H, R, OT):
    """ops.rnn_tanh_backward_step, R ragged (and the PP-hard row count): dz, dh_out with and without row_keep and a detach point,
    in place, and the bias partials, against float64."""
    from ic3net_amd import ops
    gen = torch.Generator(device='cuda').manual_seed(R + H)
    h = torch.tanh(_rn(gen, R, H)).float()
    dh_in = _rn(gen, R, H).float()
    dhead, w_heads = _rn(gen, R, OT).float(), (_rn(gen, OT, H) / H ** 0.5).float()
    a2 = (_rn(gen, H, H) / H ** 0.5).float()
    keep = (torch.rand(R, device='cuda', generator=gen) < 0.6).float()
    parts = torch.empty((ops.rnn_backward_partials(R, H), H), device='cuda')
    for cut, detached in ((False, False), (True, False), (False, True)):
        dh = (0.0 if detached else dh_in.double()) + dhead.double() @ w_heads.double()
        want_dz = dh * (1 - h.double() ** 2)
        want_out = (want_dz @ a2.double()) * (keep.double()[:, None] if cut else 1.0)
        dz, out = torch.full((R, H), float('nan'), device='cuda'), torch.full((R, H), float('nan'), device='cuda')
        ops.rnn_tanh_backward_step(None if detached else dh_in, h, dhead, w_heads, a2, dz, out, parts,
                                   out_scale=keep if cut else None)
        assert float((dz.double() - want_dz).abs().max()) <= 2e-6 * max(1.0, float(want_dz.abs().max()))
        assert float((out.double() - want_out).abs().max()) <= 4e-6 * max(1.0, float(want_out.abs().max()))
        np.testing.assert_allclose(parts.double().sum(0).cpu().numpy(), want_dz.sum(0).cpu().numpy(), rtol=1e-5,
                                   atol=1e-5 * R ** 0.5)
    buf = dh_in.clone()
    ops.rnn_tanh_backward_step(buf, h, dhead, w_heads, a2, dz, buf, parts, out_scale=keep)
    want = ((dh_in.double() + dhead.double() @ w_heads.double()) * (1 - h.double() ** 2)) @ a2.double() * keep.double()[:, None]
    assert float((buf.double() - want).abs().max()) <= 4e-6 * max(1.0, float(want.abs().max()))


@pytest.mark.parametrize("H,Q", [(64, 1000), (128, 16 * 37 + 5), (128, 4 * 81920 + 11)])
def test_window_weight_grad_against_float64(H, Q):
    """ops.rnn_weight_grad at a ragged Q, with row_live: dA2 = dz^T (row_live h_prev) against float64, accumulated."""
    from ic3net_amd import ops
    gen = torch.Generator(device='cuda').manual_seed(Q)
    dz, hp = _rn(gen, Q, H).float(), _rn(gen, Q, H).float()
    live = (torch.rand(Q, device='cuda', generator=gen) < 0.7).float()
    want = dz.double().t() @ (hp.double() * live.double()[:, None])
    dA = torch.zeros((H, H), device='cuda')
    ops.rnn_weight_grad(dz, hp, dA, row_live=live, accumulate=False)
    tol = 2e-6 * float(want.abs().max()) * max(1.0, Q ** 0.5 / 16)
    assert float((dA.double() - want).abs().max()) <= tol
    ops.rnn_weight_grad(dz, hp, dA, row_live=live, accumulate=True)
    assert float((dA.double() - 2 * want).abs().max()) <= 2 * tol


def _recorded(wl, E, T, collect=False, gap=3, **over):
    import bench
    tr, a = bench.build_trainer(wl, E, 3, 0, 0, **over)
    a.max_steps, a.batch_size = T, E * T * (2 if collect else 1)
    a.detach_gap = gap
    a.entr, a.value_coeff, a.gamma, a.normalize_rewards, a.advantages_per_action = 0.01, 0.01, 0.9, True, False
    a.auto_reset = collect
    assert tr._native_update()
    tr._records = []
    batch, _ = tr.run_batch(0)
    recs = tr._records
    tr._records = None
    return tr, a, batch, recs


def _paths(monkeypatch):
    from ic3net_amd import bptt
    seen = []
    for name in ('_backward_window_rnn', '_backward_episode_baseline', '_backward_episode_standin'):
        orig = getattr(bptt, name)

        def spy(*args, _o=orig, _n=name, **kw):
            seen.append(_n)
            return _o(*args, **kw)
        monkeypatch.setattr(bptt, name, spy)
    return seen


def _grads(tr, batch, recs, native_loop):
    tr.args.bptt_native_loop = native_loop
    tr.optimizer.zero_grad()
    tr.compute_grad_native(batch, recs)
    torch.cuda.synchronize()
    return {k: p.grad.clone() for k, p in tr.policy_net.named_parameters() if p.grad is not None}


def _agree(g1, g0, rel=1e-5):
    assert g1.keys() == g0.keys()
    for k in g0:
        err = float((g1[k] - g0[k]).abs().max())
        assert err <= rel * max(1e-3, float(g0[k].abs().max())), (k, err, float(g0[k].abs().max()))


@pytest.mark.parametrize("collect", [False, True])
@pytest.mark.parametrize("hid", [64, 128])
def test_window_equals_the_loop_on_the_same_record(monkeypatch, hid, collect):
    """The window path and the per-step loop (bptt_native_loop=False) on ONE record: lock-step with detach points inside the
    window (detach_gap 3, T 8), and collection mode over two windows with the carry between them.  (The window path first: the
    loop zeroes the rows of starting envs in the record as it goes.)"""
    seen = _paths(monkeypatch)
    tr, a, batch, recs = _recorded('pp_hard_iric_tanh', 64, 8, collect=collect, hid_size=hid)
    assert len(recs) == (2 if collect else 1)
    g1 = _grads(tr, batch, recs, True)
    assert seen == ['_backward_window_rnn'] * len(recs)
    del seen[:]
    g0 = _grads(tr, batch, recs, False)
    assert seen == ['_backward_episode_baseline'] * len(recs)
    _agree(g1, g0)


def test_two_passes_are_bit_identical():
    """Two backward passes over the same record give bit-identical a2_w, a2_b and carry (no float atomics in the new launches)."""
    from ic3net_amd import bptt
    tr, a, batch, recs = _recorded('pp_hard_iric_tanh', 256, 8, collect=True)
    _, d_out = bptt.loss_gradients(a, batch, recs)
    net, raw, rec = tr.policy_net, tr.env.env, recs[-1]
    outs = []
    with torch.no_grad():
        for _ in range(2):
            acc = bptt.new_accumulators(net)
            carry = bptt._backward_window_rnn(a, net, raw, rec, d_out[d_out.shape[0] - rec.n:], acc, None)
            torch.cuda.synchronize()
            outs.append((acc['a2_w'].clone(), acc['a2_b'].clone(), carry[0].clone()))
    for x, y in zip(*outs):
        assert torch.equal(x, y)
    assert float(outs[0][0].abs().max()) > 0 and float(outs[0][2].abs().max()) > 0


@pytest.mark.parametrize("env_name,hid", [("predator_prey", 64), ("traffic_junction", 64), ("predator_prey", 128),
                                          ("traffic_junction", 128)])
def test_native_update_matches_autograd(monkeypatch, env_name, hid):
    """A whole update of models.RNN (tanh recurrence) through the window path against loss.backward() through the autograd rollout
    replaying the same actions — detach points inside the episode, entropy term and reward normalisation on (the shape of
    test_trainer_gpu.py's baseline test)."""
    from ic3net_amd import data, models, trainer as trmod
    from ic3net_amd.action_utils import parse_action_args
    from test_trainer_gpu import build_args
    seen = _paths(monkeypatch)
    T, E = 12, 9
    flags = dict(nagents=3, dim=5, vision=1, hid_size=hid, recurrent=True, rnn_type='MLP', detach_gap=5, mean_ratio=0.5, gamma=0.95,
                 normalize_rewards=True, entr=0.01, value_coeff=0.01)
    if env_name == "traffic_junction":
        flags.update(nagents=5, dim=6, difficulty='easy', add_rate_min=0.4, add_rate_max=0.4)

    def make():
        a = build_args(env_name, dict(flags), flags['nagents'], T, E, 7)
        a.env_id_offset = 0
        env = data.init(env_name, a, False)
        a.num_actions, a.dim_actions, a.num_inputs = [env.num_actions], env.dim_actions, env.observation_dim
        a.continuous = False
        a.batch_size = E * T
        parse_action_args(a)
        torch.manual_seed(0)
        return trmod.Trainer(a, models.RNN(a, a.num_inputs).cuda(), env), a
    tr, a = make()
    assert tr._native_update()
    tr._records = []
    batch, _ = tr.run_batch(0)
    tr.optimizer.zero_grad()
    s1 = tr.compute_grad_native(batch, tr._records)
    tr._records = None
    assert seen and set(seen) == {'_backward_window_rnn'}
    g1 = {k: p.grad.clone() for k, p in tr.policy_net.named_parameters() if p.grad is not None}
    tape = torch.stack(batch.action).clone()
    tr2, a2 = make()

    def taped(args, action_out, clock, out=None):
        out.copy_(tape[clock.t])
        return out
    orig = trmod.select_action
    trmod.select_action = taped
    try:
        a2.rollout_grad = True
        batch2, _ = tr2.run_batch(0)
        tr2.optimizer.zero_grad()
        s2 = tr2.compute_grad(batch2)
    finally:
        trmod.select_action = orig
    for k in ("action_loss", "value_loss", "entropy"):
        np.testing.assert_allclose(s1[k], s2[k], rtol=2e-4, atol=1e-4, err_msg=k)
    g2 = {k: p.grad for k, p in tr2.policy_net.named_parameters() if p.grad is not None}
    assert set(g1) == set(g2)
    for k in g1:
        scale = max(float(g2[k].abs().max()), 1e-6)
        np.testing.assert_allclose(g1[k].cpu().numpy() / scale, g2[k].cpu().numpy() / scale, rtol=0, atol=5e-4, err_msg=k)


def test_window_at_the_benchmark_geometry(monkeypatch):
    """pp_hard_iric_tanh at E = 8192 (81 920 agent rows: 1280 row tiles, the persistent grid, 6-column heads) over a short window
    (T = 6, detach_gap 3) — the window path against the loop on the same record."""
    seen = _paths(monkeypatch)
    tr, a, batch, recs = _recorded('pp_hard_iric_tanh', 8192, 6)
    g1 = _grads(tr, batch, recs, True)
    g0 = _grads(tr, batch, recs, False)
    assert seen == ['_backward_window_rnn', '_backward_episode_baseline']
    _agree(g1, g0)


def test_dispatch(monkeypatch):
    """The window path for pp_hard_iric_tanh; hid 32, bptt_native_loop=False, models.MLP (IC) and the LSTM RNN keep their paths."""
    seen = _paths(monkeypatch)
    cases = [(dict(), True, '_backward_window_rnn'), (dict(hid_size=32), True, '_backward_episode_baseline'),
             (dict(), False, '_backward_episode_baseline')]
    for over, loop, want in cases:
        tr, a, batch, recs = _recorded('pp_hard_iric_tanh', 16, 4, **over)
        del seen[:]
        _grads(tr, batch, recs, loop)
        assert seen == [want], (over, loop, seen)
    tr, a, batch, recs = _recorded('pp_hard_ic', 16, 4)
    del seen[:]
    _grads(tr, batch, recs, True)
    assert seen == ['_backward_episode_baseline']
    tr, a, batch, recs = _recorded('pp_hard_iric', 16, 4)
    del seen[:]
    _grads(tr, batch, recs, True)
    assert seen == ['_backward_episode_standin']


def test_heads_gradient_is_joined_when_the_backward_raises():
    """bptt._heads_grad_beside (both window drivers issue their chain inside it): the heads' gradient forked onto the side stream is
    waited for by the current stream on the way out even when the body raises — the caller releases the record next.  The side
    stream is kept busy first, so the pass is still pending when the body raises: once the CURRENT stream is synchronised the side
    stream has nothing left, and the heads' accumulators are those of a run whose body did not raise, bit for bit."""
    from ic3net_amd import bptt
    tr, a, batch, recs = _recorded('pp_hard_iric_tanh', 64, 8)
    _, d_out = bptt.loss_gradients(a, batch, recs)
    net, rec = tr.policy_net, recs[0]
    T, R, H = rec.n, rec.hs.shape[1], rec.hs.shape[2]
    dev = rec.hs.device
    side = bptt._SIDE_STREAMS.setdefault(dev.index, torch.cuda.Stream(device=dev))
    busy = torch.randn(4096, 4096, device=dev)

    class Boom(Exception):
        pass

    def run(fail):
        acc = bptt.new_accumulators(net)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            for _ in range(30):
                busy @ busy
        try:
            with torch.no_grad(), bptt._heads_grad_beside(a, rec, d_out, acc, T, R, H):
                assert bptt._SIDE_STREAMS[dev.index] is side
                if fail:
                    raise Boom()
        except Boom:
            assert fail
        else:
            assert not fail
        torch.cuda.current_stream(dev).synchronize()
        assert side.query(), "the current stream did not wait for the side stream"
        return acc['w_heads'].clone(), acc['b_heads'].clone()

    w0, b0 = run(False)
    w1, b1 = run(True)
    assert float(w0.abs().max()) > 0 and float(b0.abs().max()) > 0
    assert torch.equal(w1, w0) and torch.equal(b1, b0)
