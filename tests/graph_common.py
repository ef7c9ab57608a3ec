"""Graph capture and replay of the stream entry points, stated once for
tests/test_gpu_graph_replay.py (in the style of tests/checks.py).

include/hc_trifocal.h promises that every entry point that takes a stream never
allocates, copies to or from the host or synchronises, so that a caller can
record its launches once and replay them on new data.  capture() records a
callable under torch.cuda.graph with the default capture error mode ("global"),
in which every such host call on any thread fails the capture: "relaxed" would
hide exactly the calls these tests are for.

Rules of a capture here (they keep a shared GPU safe, and a replay honest):
  * exactly one capture stream: nothing inside a capture forks or joins another
    stream, so no graph has parallel branches;
  * one capture at a time, in this process: no capture in a fresh subprocess;
  * GPU_MAX_HW_QUEUES and every other environment variable are left alone;
  * a graph is destroyed only after a torch.cuda.synchronize() (release());
  * launches inside the capture pass no stream: torch.cuda.current_stream() is
    then the capture stream;
  * tracking launches pass an explicit, already sized workspace
    (tracker.new_workspace(N) or new_workspace()): DeviceTracker.launch
    synchronises when it grows its default workspace;
  * the testing hooks (checks.launch_mode) are read when a launch is recorded:
    they are set around capture() only, never during a replay.

Buffers.  An in/out buffer (the tracks, found, batch_index, found_ticks,
joint_inliers) is reset by nodes inside the graph: the reset_tracks copies and
fills are captured with the launch.  A pure output buffer is filled with the
byte 0xA5 from outside the graph before every replay (poison()), so a replay
that did nothing cannot pass on the previous replay's results.  Between replays
only device buffer contents change (load()): no host struct, pointer or size.
"""
import numpy as np

POISON_BYTE = 0xA5


class Captured:
    """A recorded graph with what its enqueue returned: the output tensors are
    held for the life of the graph (they live in the graph's memory pool)."""

    def __init__(self, graph, out):
        self.graph, self.out = graph, out

    def replay(self):
        """Enqueue one replay on the current stream (no synchronisation)."""
        self.graph.replay()


def capture(enqueue):
    """Run enqueue() once eagerly and synchronise (the warm-up: it fills the
    launcher's occupancy cache and loads the code objects outside the capture),
    then record enqueue() under torch.cuda.graph in the default "global" error
    mode.  Returns (Captured, what the recorded enqueue() returned)."""
    import torch
    enqueue()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = enqueue()
    torch.cuda.synchronize()
    return Captured(g, out), out


def release(*captured):
    """Destroy graphs, after a device-wide synchronisation."""
    import torch
    torch.cuda.synchronize()
    for c in captured:
        c.graph.reset()
        c.out = None


def _tensors(items):
    import torch
    for t in items:
        if t is None:
            continue
        if isinstance(t, torch.Tensor):
            yield t
        else:
            yield from _tensors(t)


def poison(*tensors):
    """Fill pure output buffers (tensors, or nested tuples / lists of them; None
    is skipped) with the byte 0xA5, from outside the graph."""
    import torch
    for t in _tensors(tensors):
        assert t.is_contiguous(), "poison: a contiguous buffer"
        t.view(torch.uint8).fill_(POISON_BYTE)


def is_poisoned(t):
    """Whether every byte of t still is the poison byte."""
    b = t.cpu().numpy().view(np.uint8)
    return bool((b == POISON_BYTE).all())


def load(dst, src):
    """Overwrite the device buffer dst in place with the host array (or device
    tensor) src: the only thing that changes between two replays."""
    import torch
    if not isinstance(src, torch.Tensor):
        src = torch.from_numpy(np.ascontiguousarray(src))
    assert tuple(src.shape) == tuple(dst.shape) and src.dtype == dst.dtype, (src.shape, dst.shape, src.dtype, dst.dtype)
    dst.copy_(src)


def raw(t):
    """The bytes of a device tensor."""
    return t.cpu().numpy().tobytes()
