"""graphs.capture on CPU, with torch.cuda.CUDAGraph / torch.cuda.graph replaced by fakes: the body runs once inside the
capture context with the cyclic collector off, the collector is put back as it was (after a return and after a raise),
exceptions propagate unchanged and the pool is passed through."""
import gc

import pytest
import torch

from xuanpolicy_amd import graphs


class _FakeGraph:
    pass


@pytest.fixture
def fake(monkeypatch):
    """Installs the fakes; yields the log of the capture contexts: [graph, pool, "enter" | "exit" | exception type]."""
    log = []

    class _FakeCapture:
        def __init__(self, g, pool=None):
            self.entry = [g, pool, None]
            log.append(self.entry)

        def __enter__(self):
            self.entry[2] = "enter"

        def __exit__(self, exc_type, exc, tb):
            self.entry[2] = "exit" if exc_type is None else exc_type
            return False

    monkeypatch.setattr(torch.cuda, "CUDAGraph", _FakeGraph)
    monkeypatch.setattr(torch.cuda, "graph", _FakeCapture)
    was = gc.isenabled()
    yield log
    (gc.enable if was else gc.disable)()


@pytest.mark.parametrize("enabled", [True, False])
def test_capture_runs_body_once_with_collector_off(fake, enabled):
    (gc.enable if enabled else gc.disable)()
    seen = []

    def body():
        seen.append((len(fake), fake[-1][2], gc.isenabled()))
        return "result"
    pool = object()
    g, result = graphs.capture(body, pool=pool)
    assert seen == [(1, "enter", False)]          # once, inside the context, collector off
    assert isinstance(g, _FakeGraph) and result == "result"
    assert fake == [[g, pool, "exit"]]            # one capture, of the returned graph, in the given pool
    assert gc.isenabled() == enabled              # the prior state, not unconditionally on


@pytest.mark.parametrize("enabled", [True, False])
def test_capture_raising_body_propagates_and_restores_collector(fake, enabled):
    (gc.enable if enabled else gc.disable)()
    err = RuntimeError("cannot be captured")
    seen = []

    def body():
        seen.append(gc.isenabled())
        raise err
    with pytest.raises(RuntimeError) as info:
        graphs.capture(body)
    assert info.value is err and seen == [False]
    assert len(fake) == 1 and fake[0][1] is None and fake[0][2] is RuntimeError   # the context saw it and ended
    assert gc.isenabled() == enabled


def test_capture_default_pool_is_none(fake):
    graphs.capture(lambda: None)
    assert fake[0][1] is None
