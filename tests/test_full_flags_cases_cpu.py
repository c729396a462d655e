"""CPU: the case table of tests/test_full_flags_update_gpu.py keeps up with ic3net_amd.main._ENGINE_FLAGS — a path switch added
there fails here until full_flags_cases.FULL_FLAGS sets it and a row names it as the reason for its expected path.  No GPU, no
library load."""
from full_flags_cases import CASES, COUNTERS, FULL_FLAGS, NOT_PATH_SWITCHES

# the engine flags that choose no path of the update: the env count, the device, graph replay of rollouts that feed no update,
# TunableOp, the collective backend
EXCLUDED = ('nenvs', 'device', 'hip_graph', 'tune_gemm', 'dist_backend')


def _engine_flags():
    from ic3net_amd import main
    return [name for name, _, _ in main._ENGINE_FLAGS]


def test_every_path_switch_is_in_the_full_setting():
    assert tuple(NOT_PATH_SWITCHES) == EXCLUDED
    names = _engine_flags()
    assert set(EXCLUDED) <= set(names)
    switches = [n for n in names if n not in EXCLUDED]
    assert sorted(switches) == sorted(FULL_FLAGS), "a path switch without an entry in FULL_FLAGS (or the reverse)"
    assert all(bool(v) for v in FULL_FLAGS.values()), "the full setting turns every switch on"


def test_every_path_switch_is_the_reason_for_some_row():
    named = set()
    for c in CASES:
        assert c['because'] and set(c['because']) <= set(FULL_FLAGS), (c['name'], c['because'])
        named |= set(c['because'])
    assert named == set(FULL_FLAGS), "switches no row's expected path is written from: %r" % sorted(set(FULL_FLAGS) - named)


def test_rows_are_unique_name_a_mode_and_expect_every_counter():
    names = [c['name'] for c in CASES]
    assert len(names) == len(set(names))
    keys = [(c['row'], c['hid'], c['mode']) for c in CASES]
    assert len(keys) == len(set(keys))
    for c in CASES:
        assert c['mode'] in ('lock-step', 'collection'), c['name']
        assert sorted(c['expect']) == sorted(COUNTERS), c['name']
        assert any(c['expect'].values()), c['name']
    rows = {c['row'] for c in CASES}
    assert rows >= {'ic3', 'ic3-tj', 'ic3-wide', 'ic3-p2', 'ic3-p3s', 'ic3-p2-wide', 'zero-comm', 'iric-lstm', 'iric-tanh', 'ic-mlp',
                    'mlp2', 'twin'}
    assert any(c['mode'] == 'collection' for c in CASES)
    assert len([c for c in CASES if c['normalize_rewards']]) == 1
