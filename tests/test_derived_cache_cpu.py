"""The derived-weights caches of comm.CommNetMLP (_fused_cache / _commnet_cache, one mechanism: CommNetMLP._derived) on the
CPU, with the pack ops of the non-recurrent cache stubbed in torch: ONE build per weight version — a call at an unchanged
version builds nothing and writes no parameter —, and a new version is copied into the old tensors (captured graphs hold
their addresses; cache_generation counts address changes only)."""
import argparse

import pytest
import torch


def _args(H, recurrent, passes):
    return argparse.Namespace(
        hid_size=H, recurrent=recurrent, rnn_type='LSTM' if recurrent else 'MLP', nagents=4, comm_mode='avg',
        comm_passes=passes, comm_mask_zero=False, comm_init='uniform', hard_attn=True, share_weights=False,
        continuous=False, naction_heads=[5, 2], commnet=True, mean_ratio=0)


@pytest.mark.parametrize("recurrent", [False, True], ids=["commnet_cache", "fused_cache"])
def test_one_build_per_weight_version_and_refresh_in_place(recurrent, monkeypatch):
    from ic3net_amd import ops
    from ic3net_amd.comm import CommNetMLP
    monkeypatch.setattr(ops, 'commnet_pack', lambda cw, fw, cb, fb: (
        torch.stack([torch.cat([c, f], 1) for c, f in zip(cw, fw)]).detach().clone(),
        torch.stack([c + f for c, f in zip(cb, fb)]).detach().clone()))
    monkeypatch.setattr(ops, 'commnet_pack_split', lambda cw, fw: torch.stack([torch.cat([c, f], 1) for c, f in zip(cw, fw)]).detach() * 2)
    torch.manual_seed(0)
    net = CommNetMLP(_args(20, recurrent, 1 if recurrent else 2), 11)        # (hid 20: no kernel size, so no packed layouts of the library)
    cache = net._fused_cache if recurrent else net._commnet_cache
    builds = [0]
    heads_cat = net._heads_cat

    def counted():                                                            # (every build of either cache concatenates the heads once)
        builds[0] += 1
        return heads_cat()
    monkeypatch.setattr(net, '_heads_cat', counted)

    def versions():
        return [q._version for q in net.parameters()]

    v0 = versions()
    first = cache()
    for _ in range(3):
        assert cache() is first
    assert builds[0] == 1 and versions() == v0 and net.cache_generation == 1
    ptrs = {k: v.data_ptr() for k, v in first.items() if v is not None}
    shared = set(q.untyped_storage().data_ptr() for q in net.parameters())
    assert not any(v.untyped_storage().data_ptr() in shared for v in first.values() if v is not None)   # the cache owns its tensors

    for step in range(2):                                                     # two weight versions, as two optimizer steps make them
        with torch.no_grad():
            for q in net.parameters():
                q.mul_(0.5).add_(0.01)
        v1 = versions()
        if step:
            net.refresh_derived()                                             # (what Trainer.begin_episode calls before replays)
        for _ in range(5):
            assert cache() is first
        assert builds[0] == 2 + step, "a call at an unchanged weight version built the cache again"
        assert versions() == v1, "refreshing the cache wrote a parameter"
        assert net.cache_generation == 1 and {k: v.data_ptr() for k, v in first.items() if v is not None} == ptrs
        assert torch.equal(first['wt'], net.encoder.weight.detach().t())
        bias = net.encoder.bias + net.C_modules[0].bias if recurrent else net.encoder.bias
        assert torch.equal(first['enc_bias'], bias.detach())
        assert torch.equal(first['b_heads'][:5], net.heads[0].bias.detach())
