"""CPU: the engine flag --window_launch_collection (ic3net_amd.main) — known to the parser, an int, off by default, beside the switches it
acts with; and what the Trainer makes of it before any launch: a collection window is asked for only with the flag set."""
from types import SimpleNamespace

from ic3net_amd import main
from ic3net_amd.trainer import Trainer


def parse(argv):
    argv = ['main.py'] + argv
    return main.build_parser(argv).parse_args(argv[1:])


def test_the_parser_knows_the_flag_and_it_is_off_by_default():
    a = parse([])
    assert a.window_launch_collection == 0 and isinstance(a.window_launch_collection, int)
    assert a.window_launch is False and a.multipass_window_collection == 0          # no default moved
    a = parse(['--window_launch', '--window_launch_collection', '1', '--env_name', 'predator_prey'])
    assert a.window_launch is True and a.window_launch_collection == 1
    assert ('window_launch_collection', int, 0) in main._ENGINE_FLAGS


def _asks(**flags):
    """Trainer._window_launch_ok on a stand-in that reaches the first question behind the auto-reset exclusion (store_states)."""
    seen = []

    class Args(SimpleNamespace):
        @property
        def store_states(self):
            seen.append('store_states')
            return True
    tr = Trainer.__new__(Trainer)
    tr.args = Args(window_launch=True, **flags)
    tr._rec, tr.env = object(), SimpleNamespace(env=SimpleNamespace(auto_max_steps=8 if flags.get('auto_reset') else 0))
    assert Trainer._window_launch_ok(tr) is False
    return bool(seen)


def test_a_collection_window_is_considered_only_with_the_flag():
    assert _asks(auto_reset=False)                                                  # lock-step: as before
    assert not _asks(auto_reset=True)                                               # collection mode keeps the per-step path ...
    assert not _asks(auto_reset=True, window_launch_collection=0)
    assert _asks(auto_reset=True, window_launch_collection=1)                       # ... unless the flag is set
