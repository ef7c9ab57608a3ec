"""Keeps the graph-replay table complete (CPU): every entry point under
include/ that takes a stream is either recorded and replayed by
tests/test_gpu_graph_replay.py or a test hook whose header comment says that it
blocks.  A new entry point fails here until it gets a capture case or a
documented exemption."""
import os
import re

from conftest import ROOT

INCLUDE = os.path.join(ROOT, "include")

# Test hooks that synchronise by design: not capturable, and their header comments say so
BLOCKING = ("hc_trifocal_ring_check_test", "hc_cgesv_30x30_struct_batched", "hc_cgesv_30x30_variant_batched",
            "hc_trifocal_eval_variant_batched")


def _headers():
    out = []
    for d, _, files in os.walk(INCLUDE):
        out += [os.path.join(d, f) for f in files if f.endswith((".h", ".hpp"))]
    return sorted(out)


def _stream_prototypes():
    """{name: the comment that precedes its prototype} of every function under
    include/ with an hcStream parameter."""
    out = {}
    for path in _headers():
        src = open(path).read()
        # comments blanked out (same length), so that a prototype is looked for in code only
        code = re.sub(r"/\*.*?\*/", lambda m: re.sub(r"[^\n]", " ", m.group(0)), src, flags=re.S)
        for m in re.finditer(r"\b(hc_\w+)\s*\(([^()]*)\)\s*;", code):
            if not re.search(r"\bhcStream\b", m.group(2)):
                continue
            comments = [c for c in re.finditer(r"/\*.*?\*/", src[:m.start()], flags=re.S)]
            assert m.group(1) not in out, f"{m.group(1)} is declared twice"
            out[m.group(1)] = comments[-1].group(0) if comments else ""
    return out


def test_every_stream_entry_point_is_replayed_or_documented_as_blocking():
    import test_gpu_graph_replay as T
    protos = _stream_prototypes()
    assert len(protos) >= 25, sorted(protos)
    assert len(set(T.CAPTURED)) == len(T.CAPTURED), "a name is listed twice"
    assert not set(T.CAPTURED) & set(BLOCKING)
    assert set(protos) == set(T.CAPTURED) | set(BLOCKING), \
        (sorted(set(protos) - set(T.CAPTURED) - set(BLOCKING)), sorted((set(T.CAPTURED) | set(BLOCKING)) - set(protos)))
    # every listed name is recorded by a test of the file, and nothing else is
    assert set(T.RECORDED_BY) == set(T.CAPTURED), sorted(set(T.CAPTURED) ^ set(T.RECORDED_BY))
    for name, tests in T.RECORDED_BY.items():
        for t in tests:
            assert callable(getattr(T, t)), (name, t)


def test_the_exempt_hooks_say_that_they_block():
    protos = _stream_prototypes()
    for name in BLOCKING:
        assert "lock" in protos[name], f"{name}: its comment does not say that it blocks"


def test_the_parser_sees_only_prototypes_with_a_stream():
    protos = _stream_prototypes()
    assert "hc_trifocal_2op1p_30x30_track" in protos and "hc_trifocal_pose_refine_topk_grouped" in protos
    for name in ("hc_trifocal_workspace_status", "hc_trifocal_read_timestamps", "hc_pose_merge_joint",
                 "hc_shared_flag_create"):
        assert name not in protos
