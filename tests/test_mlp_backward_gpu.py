"""GPU: the IC baseline's (models.MLP) window backward (ic3_mlp_backward, bptt._backward_window_mlp) — its kernel against float64
(ragged, several tiles per workgroup, rings beyond 4 GB), run-to-run identity, whole updates against the per-step loop
(bptt._backward_episode_baseline) on the same record, against autograd through the rollout replaying the same actions and against
the reference's fp64 gradients of a committed fixture, the benchmark geometry, and which path each policy takes."""
import ast

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_rnn_backward_gpu import _agree, _grads, _recorded  # noqa: E402  (the sibling's helpers: same shapes, same bar)


def _rn(gen, *s):
    return torch.randn(*s, device='cuda', generator=gen, dtype=torch.float64)


def _reference(e, h, dhead, w_heads, a2):
    """x1 = tanh(e); dz = (d . W_heads)(1 - h^2); de = (dz . A2 + dz)(1 - x1^2), in float64"""
    x1 = torch.tanh(e.double())
    dz = (dhead.double() @ w_heads.double()) * (1 - h.double() ** 2)
    de = (dz @ a2.double() + dz) * (1 - x1 ** 2)
    return x1, dz, de


def _bars(got, want, rel):
    err, ref = float((got.double() - want).abs().max()), float(want.abs().max())
    print("max error %.3e against %.3e x max(1, %.3e)" % (err, rel, ref))
    assert err <= rel * max(1.0, ref)


@pytest.mark.parametrize("H,Q,OT", [(64, 333, 6), (128, 64 * 600 + 5, 16)])
def test_mlp_step_against_float64(H, Q, OT):
    """ops.mlp_backward_step against float64 with the host test's bars: Q ragged with one tile per workgroup, and 601 tiles on at
    most 256 workgroups (a workgroup walks several tiles, the ragged tile is not its first): x1 written over e, dz, de, the bias
    partials, and accumulation onto them."""
    from ic3net_amd import ops
    gen = torch.Generator(device='cuda').manual_seed(Q + H)
    e = _rn(gen, Q, H).float()
    h = torch.tanh(_rn(gen, Q, H)).float()
    dhead, w_heads = _rn(gen, Q, OT).float(), (_rn(gen, OT, H) / H ** 0.5).float()
    a2 = (_rn(gen, H, H) / H ** 0.5).float()
    want_x1, want_dz, want_de = _reference(e, h, dhead, w_heads, a2)
    nparts = ops.mlp_backward_partials(Q, H)
    assert 1 <= nparts <= min((Q + 63) // 64, 512)
    parts = torch.full((nparts, H), float('nan'), device='cuda')
    for accumulate in (False, True):
        before = parts.double().sum(0)
        x1 = e.clone()
        dz, de = torch.full((Q, H), float('nan'), device='cuda'), torch.full((Q, H), float('nan'), device='cuda')
        assert ops.mlp_backward_step(x1, h, dhead, w_heads, a2, dz, de, parts, accumulate=accumulate) == nparts
        _bars(x1, want_x1, 2e-6)
        _bars(dz, want_dz, 2e-6)
        _bars(de, want_de, 4e-6)
        want_sum = want_dz.sum(0) + (before if accumulate else 0.0)
        np.testing.assert_allclose(parts.double().sum(0).cpu().numpy(), want_sum.cpu().numpy(), rtol=1e-5, atol=1e-4)


def test_mlp_step_with_rings_beyond_4_gb():
    """Q = 2^23 + 197 rows at hid 128: every ring is 4 GB + 100 KB, so a 32-bit byte offset wraps inside it.  Filled on the
    device; compared with float64 on the first 128 rows, the 128 rows straddling byte offset 2^32 and the last 197 rows (the
    partials are left unchecked here)."""
    from ic3net_amd import ops
    H, OT, Q = 128, 6, 2 ** 23 + 197
    gen = torch.Generator(device='cuda').manual_seed(5)
    x1 = torch.empty((Q, H), device='cuda').normal_(generator=gen)
    h = torch.empty((Q, H), device='cuda').uniform_(-0.95, 0.95, generator=gen)
    dhead = torch.empty((Q, OT), device='cuda').normal_(generator=gen)
    w_heads, a2 = (_rn(gen, OT, H) / H ** 0.5).float(), (_rn(gen, H, H) / H ** 0.5).float()
    mid = 2 ** 32 // (H * 4)
    spans = [(0, 128), (mid - 64, mid + 64), (Q - 197, Q)]
    e_rows = [x1[a:b].clone() for a, b in spans]
    dz = torch.empty((Q, H), device='cuda')
    de = torch.empty((Q, H), device='cuda')
    for (a, b) in spans:
        dz[a:b] = float('nan')
        de[a:b] = float('nan')
    parts = torch.empty((ops.mlp_backward_partials(Q, H), H), device='cuda')
    ops.mlp_backward_step(x1, h, dhead, w_heads, a2, dz, de, parts)
    for (a, b), e in zip(spans, e_rows):
        want_x1, want_dz, want_de = _reference(e, h[a:b], dhead[a:b], w_heads, a2)
        _bars(x1[a:b], want_x1, 2e-6)
        _bars(dz[a:b], want_dz, 2e-6)
        _bars(de[a:b], want_de, 4e-6)


def _paths(monkeypatch):
    from ic3net_amd import bptt
    seen = []
    for name in ('_backward_window_mlp', '_backward_window_rnn', '_backward_episode_baseline', '_backward_episode_commnet',
                 '_backward_episode_standin'):
        orig = getattr(bptt, name)

        def spy(*args, _o=orig, _n=name, **kw):
            seen.append(_n)
            return _o(*args, **kw)
        monkeypatch.setattr(bptt, name, spy)
    return seen


WINDOW = ['_backward_episode_baseline', '_backward_window_mlp']    # (the baseline driver itself hands over to the window)
LOOP = ['_backward_episode_baseline']


@pytest.fixture(scope="module")
def two_passes():
    """Two backward passes of bptt._backward_window_mlp over one record (computed once for the cases below)."""
    from ic3net_amd import bptt
    tr, a, batch, recs = _recorded('pp_hard_ic', 256, 8)
    _, d_out = bptt.loss_gradients(a, batch, recs)
    net, raw, rec = tr.policy_net, tr.env.env, recs[-1]
    assert bptt._mlp_window_ok(a, net, raw, rec, d_out)
    outs = []
    with torch.no_grad():
        for _ in range(2):
            acc = bptt.new_accumulators(net)
            bptt._backward_window_mlp(a, net, raw, rec, d_out[d_out.shape[0] - rec.n:], acc)
            torch.cuda.synchronize()
            outs.append({k: acc[k].clone() for k in ('a2_w', 'a2_b', 'wt', 'a1_b')})
    return outs


@pytest.mark.parametrize("key", ['a2_w', 'a2_b', 'wt', 'a1_b'])
def test_two_passes_are_bit_identical(two_passes, key):
    """Two backward passes over the same record give bit-identical a2_w, a2_b, wt and a1_b: no float atomics in the new launch, nor
    in the weight-gradient launch behind it, and the encoder's expansion through its ordered finish
    (ic3_env_encode_backward_window_finish_ordered: the plain finish adds into dWt with global float atomics, which moved `wt` by
    1.4e-6 .. 2.4e-6 on a largest entry of 12.3 between two passes on an MI355X)."""
    first, second = two_passes
    assert float(first[key].abs().max()) > 0
    diff = float((first[key] - second[key]).abs().max())
    print("%s: max difference between two passes %.3e on a largest entry of %.3e" % (key, diff, float(first[key].abs().max())))
    assert torch.equal(first[key], second[key])


@pytest.mark.parametrize("collect", [False, True])
@pytest.mark.parametrize("hid", [64, 128])
def test_window_equals_the_loop_on_the_same_record(monkeypatch, hid, collect):
    """The window path and the per-step loop (bptt_native_loop=False) on ONE record: lock-step, and collection mode over two
    windows (no state crosses a step: neither path applies a cut)."""
    seen = _paths(monkeypatch)
    tr, a, batch, recs = _recorded('pp_hard_ic', 64, 8, collect=collect, hid_size=hid)
    assert len(recs) == (2 if collect else 1)
    snaps = [r.h_fin.clone() for r in recs]
    g1 = _grads(tr, batch, recs, True)
    assert seen == WINDOW * len(recs)
    del seen[:]
    g0 = _grads(tr, batch, recs, False)
    assert seen == LOOP * len(recs)
    _agree(g1, g0)
    assert all(torch.equal(r.h_fin, s) for r, s in zip(recs, snaps))       # (the record is read, never written)


def test_window_with_the_per_step_encoder_form_equals_the_loop(monkeypatch):
    """args.enc_window=False: ic3_mlp_backward runs the encoder's first stage per step (ic3_env_encode_backward_accumulate, last
    step first) and the driver finishes with encode_backward_finish — against the loop on the same record, the same bar."""
    seen = _paths(monkeypatch)
    tr, a, batch, recs = _recorded('pp_hard_ic', 64, 8)
    a.enc_window = False
    g1 = _grads(tr, batch, recs, True)
    assert seen == WINDOW
    g0 = _grads(tr, batch, recs, False)
    _agree(g1, g0)


@pytest.mark.parametrize("wl,E,H", [("pp_hard_ic", 256, 128), ("tj_medium_commnet_mlp", 64, 64)])
def test_ordered_finish_against_float64_and_the_plain_finish(wl, E, H):
    """envs.encode_backward_window_finish_ordered on the GPU, PP-hard's and TJ-medium's grids over a window of T = 4 recorded
    states: dWt = sum_t obs_t^T g_t and dbias = sum_t sum_rows g_t against float64 from the dense observations, within
    2e-6 x max|want| x max(1, sqrt(rows) / 16) (fp32 sums of T x R terms per entry: the window weight gradient's bar); the plain
    finish on the same partials within the same bar; two calls bit-identical; the partials untouched."""
    tr, a, batch, recs = _recorded(wl, E, 4, hid_size=H)
    raw, rec = tr.env.env, recs[0]
    T, R = rec.n, raw.nenvs * raw.nagents_env
    gen = torch.Generator(device='cuda').manual_seed(E + H)
    g = torch.randn(T, R, H, device='cuda', generator=gen)
    want, wantb = 0.0, 0.0
    for t in range(T):
        obs = raw.observe_timed(rec.snaps[t]).reshape(R, -1).double()
        want = want + obs.t() @ g[t].double()
        wantb = wantb + g[t].double().sum(0)
    work = raw.encode_window_work(H)
    assert work is not None
    raw.encode_backward_window(g, rec.snaps, H, first=True)
    before = work.clone()
    dwt, db = raw.encode_backward_window_finish_ordered(H)
    dwt2, db2 = raw.encode_backward_window_finish_ordered(H)
    pw, pb = raw.encode_backward_window_finish(H)
    torch.cuda.synchronize()
    assert torch.equal(dwt, dwt2) and torch.equal(db, db2) and torch.equal(work, before)
    rel = 2e-6 * max(1.0, (T * R) ** 0.5 / 16)
    for got, ref, label in ((dwt, want, 'dWt'), (db, wantb, 'dbias'), (pw, want, 'plain dWt'), (pb, wantb, 'plain dbias')):
        err, top = float((got.double() - ref).abs().max()), float(ref.abs().max())
        print("%s: max error %.3e against %.3e x %.3e" % (label, err, rel, top))
        assert err <= rel * top


def test_window_at_the_benchmark_geometry(monkeypatch):
    """pp_hard_ic at E = 8192 (81 920 agent rows per step: the persistent grid, 6-column heads) over a short window (T = 6) —
    the window path against the loop on the same record."""
    seen = _paths(monkeypatch)
    tr, a, batch, recs = _recorded('pp_hard_ic', 8192, 6)
    g1 = _grads(tr, batch, recs, True)
    g0 = _grads(tr, batch, recs, False)
    assert seen == WINDOW + LOOP
    _agree(g1, g0)


@pytest.mark.parametrize("env_name,hid", [("predator_prey", 64), ("traffic_junction", 64), ("predator_prey", 128),
                                          ("traffic_junction", 128)])
def test_native_update_matches_autograd(monkeypatch, env_name, hid):
    """A whole update of models.MLP through the window path against loss.backward() through the autograd rollout replaying the
    same actions — entropy term and reward normalisation on (the shape of test_trainer_gpu.py's baseline test, its bars)."""
    from ic3net_amd import data, models, trainer as trmod
    from ic3net_amd.action_utils import parse_action_args
    from test_trainer_gpu import build_args
    seen = _paths(monkeypatch)
    T, E = 12, 9
    flags = dict(nagents=3, dim=5, vision=1, hid_size=hid, recurrent=False, rnn_type='MLP', detach_gap=5, mean_ratio=0.5, gamma=0.95,
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
        return trmod.Trainer(a, models.MLP(a, a.num_inputs).cuda(), env), a
    tr, a = make()
    assert tr._native_update()
    tr._records = []
    batch, _ = tr.run_batch(0)
    tr.optimizer.zero_grad()
    s1 = tr.compute_grad_native(batch, tr._records)
    tr._records = None
    assert seen and seen == WINDOW * (len(seen) // 2)
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


def test_window_matches_the_reference_gradients(monkeypatch):
    """One hop to the reference: the committed fixture grad_pp_medium_ic_mlp (hid 64, 5 agents, 20 steps, the reference's fp64
    gradients).  Its tape is replayed as test_trainer_gpu.py does — a taped rollout takes the launch chain and records no h — and
    each record's h_fin is filled here (the encoder on every snapshot, then tanh and tanh(x1 A2^T + b2 + x1) in float64, cast to
    float32); compute_grad_native then takes the window path.  Every parameter gradient and the three losses at that fixture's
    entry of GRAD_TOL (the project's floor, 4.0e-6 / 2.0e-6; the window path's own error: profiles/r08/grad_errors_mlp_window.txt)."""
    from golden_util import load
    from ic3net_amd import data, models, trainer as trmod
    from ic3net_amd.action_utils import parse_action_args
    from test_trainer_gpu import GRAD_TOL, _check_against_reference, build_args
    name, env_name = "grad_pp_medium_ic_mlp", "predator_prey"
    assert name in GRAD_TOL
    seen = _paths(monkeypatch)
    fx = load(name)
    N, T, nenv, nep, nh, seed = [int(x) for x in fx["cfg"]]
    flags = dict(ast.literal_eval(str(fx["flags"])))
    a = build_args(env_name, flags, N, T, nenv, seed)
    a.env_id_offset = 400
    env = data.init(env_name, a, False)
    a.num_actions, a.dim_actions, a.num_inputs = [env.num_actions], env.dim_actions, env.observation_dim
    parse_action_args(a)
    assert str(fx["model"]) == 'mlp' and a.hid_size == 64 and not a.recurrent
    a.continuous = False
    net = models.MLP(a, a.num_inputs)
    net.load_state_dict({k[2:]: torch.from_numpy(fx[k]).float() for k in fx.files if k.startswith("w:")})
    net = net.cuda()
    tr = trmod.Trainer(a, net, env)
    tape = fx["tape"]

    def taped(args, action_out, clock, out=None):
        out.copy_(torch.from_numpy(tape[:, clock.episode, clock.t]).permute(1, 0, 2).contiguous().int().cuda())
        return out
    orig = trmod.select_action
    trmod.select_action = taped
    try:
        a.rollout_grad = False
        a.batch_size = int(fx["num_steps"])
        assert tr._native_update()
        tr._records = []
        batch, stats = tr.run_batch(0)
        recs = tr._records
    finally:
        trmod.select_action = orig
        tr._records = None
    assert len(recs) == nep and all(r.h_fin is None for r in recs)
    raw = tr.env.env
    wt = net.affine1.weight.detach().t().contiguous()
    A2, b2 = net.affine2.weight.detach().double(), net.affine2.bias.detach().double()
    for r in recs:
        r.h_fin = torch.empty((r.n, r.rows, a.hid_size), device='cuda')
        for t in range(r.n):
            x1 = torch.tanh(raw.encode_at(r.snaps[t], wt, net.affine1.bias.detach()).reshape(r.rows, -1).double())
            r.h_fin[t] = torch.tanh(x1 @ A2.t() + b2 + x1).float()
        r.h_fin_n = r.n
    tr.optimizer.zero_grad()
    s = tr.compute_grad_native(batch, recs)
    assert seen == WINDOW * nep
    _check_against_reference(name + "/native-window", fx, s, net)


@pytest.mark.parametrize("wl,over,loop,want", [
    ("pp_hard_ic", dict(), True, WINDOW),
    ("pp_hard_ic", dict(hid_size=32), True, LOOP),
    ("pp_hard_ic", dict(), False, LOOP),                                   # (h recorded, the loop asked for at the update)
    ("pp_hard_ic", dict(bptt_native_loop=False), False, LOOP),             # (asked for before the rollout: no h recorded)
    ("pp_hard_ic", dict(mega_policy=False), True, LOOP),                   # launch-chain rollout: no h recorded
    ("pp_hard_iric_tanh", dict(), True, ['_backward_window_rnn']),
    ("tj_medium_commnet_mlp", dict(), True, ['_backward_episode_commnet']),
], ids=["ic-128", "ic-32", "ic-loop-off", "ic-loop-off-rollout", "ic-launch-chain", "iric-tanh", "commnet-mlp"])
def test_dispatch(monkeypatch, wl, over, loop, want):
    """pp_hard_ic at hid 128 takes the window; hid 32, bptt_native_loop=False and the launch-chain rollout (mega_policy=False: no h
    recorded) keep the loop; the tanh recurrence and the non-recurrent CommNet module keep their paths, and only the IC baseline's
    one-launch rollout gets an h record."""
    seen = _paths(monkeypatch)
    tr, a, batch, recs = _recorded(wl, 16, 4, **over)
    has_h = [r.h_fin is not None and r.h_fin_n == r.n for r in recs]
    assert has_h == [wl == 'pp_hard_ic' and not over] * len(recs)
    if wl != 'pp_hard_ic':
        assert all(r.h_fin is None for r in recs)
    _grads(tr, batch, recs, loop)
    assert seen == want, (wl, over, loop, seen)
