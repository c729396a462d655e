"""GPU: the update of a recurrent policy with comm_passes > 1 in COLLECTION mode (args.auto_reset: a record is a window of slots of E
streams of episodes) on the window backward, behind args.multipass_window_collection — for ONE recorded batch of several windows,
Trainer.compute_grad_native with the switch on and off: the path counters say which backward ran, the losses are equal, every
parameter's gradient agrees with the per-step loop's (tests/bptt_passes_stream_bars.py: 4 x the measured worst |window - loop| /
max |loop| per parameter); the same with every window walked in chunks of 3 slots; and the reference's own gradients for the golden
collection-mode fixture of a two-pass IC3Net, through the window path."""
import pytest
import torch

import bptt_passes_stream_ref as ref

pytestmark = pytest.mark.gpu

E, T, NWIN = 32, 8, 3


def _trainer():
    """Predator-Prey on a 3 x 3 grid with 2 predators: a random policy ends episodes within a few steps, so the windows hold episode
    ends, starts and detach points (every 5 steps of an env's own counter) at slots of their own"""
    import bench
    tr, a = bench.build_trainer("pp_easy", E, 3, 0, 0, comm_passes=2, hid_size=64, nagents=2, dim=3, vision=1, max_steps=T, detach_gap=5)
    a.auto_reset = True
    a.__dict__.update(gamma=0.95, normalize_rewards=True, entr=0.01, value_coeff=0.01, advantages_per_action=False, batch_size=NWIN * E * T)
    return tr, a


def _counters(tr):
    net = tr._kernel_net()
    return getattr(net, 'multipass_window_backwards', 0), getattr(net, 'multipass_loop_backwards', 0)


def test_collection_window_update_against_the_loop(monkeypatch):
    from ic3net_amd import bptt
    tr, a = _trainer()
    assert tr._native_update() and not getattr(a, 'multipass_window_collection', False)      # off where nobody sets it
    tr._records = []
    batch, _ = tr.run_batch(0)
    recs = tr._records
    assert len(recs) == NWIN and all(r.stream is not None and r.n == T for r in recs)
    # the batch must hold what the test is about: an episode start and a cut INSIDE a window, a cut that is no episode end's, and
    # a gradient that crosses a window border (an env whose state leaving a window's last slot is kept)
    fresh = torch.cat([r.stream['fresh'][:T] for r in recs]).view(NWIN, T, E)
    keep = torch.cat([r.stream['keep'][:T] for r in recs]).view(NWIN, T, E)
    assert bool(fresh[:, 1:].any()), "no episode starts inside a window"
    assert bool((~keep[:, :-1]).any()), "no cut inside a window"
    assert bool((~keep[:, :-1] & ~fresh[:, 1:]).any()), "no detach point inside a window"
    assert bool(keep[:-1, -1].any()) and bool((~keep[:-1, -1]).any()), "the window borders: a kept and a cut env"
    whole = bptt._backward_window_multipass

    def chunked(*args, **kw):
        return whole(*args, max_chunk_steps=3, **kw)
    grads, stats, chunk = {}, {}, {}
    for mode in ('window', 'chunks', 'loop'):                      # (the loop last: it zeroes the starting envs' rows of the records)
        a.multipass_window_collection = mode != 'loop'
        monkeypatch.setattr(bptt, '_backward_window_multipass', chunked if mode == 'chunks' else whole)
        before = _counters(tr)
        tr.optimizer.zero_grad()
        stats[mode] = tr.compute_grad_native(batch, recs)
        torch.cuda.synchronize()
        ran = tuple(x - y for x, y in zip(_counters(tr), before))
        assert ran == ((0, NWIN) if mode == 'loop' else (NWIN, 0)), "which backward ran (window, loop) in mode %s: %r" % (mode, ran)
        chunk[mode] = getattr(tr._kernel_net(), 'multipass_window_chunk', None)
        grads[mode] = {k: p.grad.clone() for k, p in tr.policy_net.named_parameters() if p.grad is not None}
    tr._records = None
    assert chunk['window'] == T and chunk['chunks'] == 3
    for mode in ('window', 'chunks'):
        for k in ("action_loss", "value_loss", "entropy"):
            assert stats[mode][k] == stats['loop'][k], (mode, k)
    g0 = grads['loop']
    missed = []
    for mode in ('window', 'chunks'):
        g1 = grads[mode]
        assert set(g1) == set(g0) and g1
        errs = {}
        for k in g0:
            scale = max(float(g0[k].abs().max()), 1e-12)
            assert bool(torch.isfinite(g1[k]).all()) and scale > 1e-9, k
            errs[k] = float((g1[k].double() - g0[k].double()).abs().max() / scale)
        try:                                                       # (both modes print their figures before either fails the test)
            ref.check('gpu/trainer-collection-pp-tiny-p2-' + mode, errs)
        except AssertionError as e:
            missed.append(str(e))
    assert not missed, missed


def test_golden_collection_fixture_through_the_window_path(monkeypatch):
    """tests/golden/gradstream_pp_tiny_ic3net_p2.npz (the reference's run_batch + compute_grad over whole episodes per env) through
    tests/test_trainer_gpu.py's collection-mode machinery with the switch on where the arguments do not carry it: the window path
    runs for every window, the losses and every parameter's gradient against the reference's at this path's own bar."""
    import numpy as np
    import test_trainer_gpu as ttg
    from ic3net_amd import bptt
    name = "gradstream_pp_tiny_ic3net_p2"
    seen = {}

    def check(label, fx, s, net):
        loss_err = max(abs(s[k] - float(fx[k])) / max(abs(float(fx[k])), 1.0) for k in ("action_loss", "value_loss", "entropy"))
        worst = 0.0
        for pname, p in net.named_parameters():
            g = fx["g:" + pname]
            if g.size == 0:
                assert p.grad is None, pname
                continue
            worst = max(worst, float(np.abs(p.grad.cpu().numpy().astype(np.float64) - g).max() / max(np.abs(g).max(), 1e-6)))
        seen.update(gradients=worst, losses=loss_err, counters=(getattr(net, 'multipass_window_backwards', 0),
                                                                getattr(net, 'multipass_loop_backwards', 0)),
                    nwin=int(fx["cfg"][3]))
    monkeypatch.setattr(bptt, 'MULTIPASS_WINDOW_COLLECTION_DEFAULT', True)
    monkeypatch.setattr(ttg, '_check_against_reference', check)
    ttg.test_collection_mode_grad_matches_reference(name, "predator_prey")
    assert seen and seen['counters'] == (seen['nwin'], 0), seen
    ref.check('gpu/fixture-' + name, dict(gradients=seen['gradients'], losses=seen['losses']))
