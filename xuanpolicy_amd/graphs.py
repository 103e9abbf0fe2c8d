"""The one place a hipGraph is recorded ("Graph capture"): every capture-time rule lives here."""
import gc

import torch


def capture(body, pool=None):
    """Record body()'s launches (recorded, not executed) into a new graph: returns (graph, body's result); an exception
    of body propagates as it is, after torch has ended the capture.  The cyclic collector is off while body runs: a
    collection started by body's own allocations could run the destructor of an unrelated graph or pool, and its HIP
    calls are not legal during a global-mode capture.  torch.cuda.graph still collects once, explicitly, on entry."""
    g = torch.cuda.CUDAGraph()
    was_enabled = gc.isenabled()
    gc.disable()
    try:
        with torch.cuda.graph(g, pool=pool):
            return g, body()
    finally:
        if was_enabled:
            gc.enable()
