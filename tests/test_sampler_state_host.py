"""The sampler's state blob (vv_sampler_state_*; Sampler.state / set_state): a sampler resumed from it delivers, bit for bit, the batches
of the one that was never interrupted.  Host only.

k = 7 batches, get, put into a fresh sampler of the same parameters, k more, against 2k uninterrupted -- for every sampler family the
golden tests name, with source and destination each serial and pipelined.  A pipelined source's ring is full when its state is read
(vv_sampler_stat 10 / 11), so the pipeline is provably ahead of the consumer whose position the blob must describe."""
import ctypes as C
import os
import re
import time

import numpy as np
import pytest

import videovector_amd as vv
from videovector_amd.engine import VVError
from videovector_amd.synth import SyntheticVideos

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VV_ERR_ARG, VV_ERR_STATE = 1, 3
K, DEPTH = 7, 3
B, CTX, NN = 8, 5, 10
DS = SyntheticVideos(seed=99, n_videos=40)


def _negatives():
    """A negative dataset of exactly max_buffer_size shots (the reference CHECKs an exact fit), rows behind the main table's."""
    n = np.full(5, 8, np.int32)
    base = DS.n_rows + np.concatenate([[0], np.cumsum(n)[:-1]]).astype(np.int64)
    return (np.arange(5000, 5005, dtype=np.int32), n, base)


FAMILIES = {
    "window_fast": dict(),
    "general_q1": dict(max_same_video_negs=6),
    "negative_dataset": dict(negatives=_negatives()),
    "rand_skip": dict(initial_cursor=17),
    "pairwise": dict(context_type="PAIRWISE"),
    "past": dict(context_type="PAST"),
    "past_q1": dict(context_type="PAST", max_same_video_negs=3),
}


def make(family, **over):
    kw = dict(batch_size=B, context_size=CTX, num_negative_samples=NN, max_buffer_size=40, negative_swap_percentage=50)
    kw.update(FAMILIES[family])
    kw.update(over)
    return vv.Sampler(DS.video_id, DS.n_shots, DS.row_base, **kw)


def take(s, n):
    return [s.next(want_last=True, want_label=True) for _ in range(n)]


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def wait_full(s):
    t0 = time.monotonic()
    while s.stat(10) - s.stat(11) < DEPTH:
        assert time.monotonic() - t0 < 20, "the pipeline did not fill its ring"
        time.sleep(0.0005)


_want = {}


def uninterrupted(family):
    if family not in _want:
        s = make(family)
        _want[family] = take(s, 2 * K)
        s.close()
    return _want[family]


@pytest.mark.parametrize("dst_pipe", [False, True], ids=["to_serial", "to_pipelined"])
@pytest.mark.parametrize("src_pipe", [False, True], ids=["from_serial", "from_pipelined"])
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_round_trip(family, src_pipe, dst_pipe):
    want = uninterrupted(family)
    a = make(family)
    if src_pipe:
        a.prefetch_start(depth=DEPTH, threads=3)
    for i, got in enumerate(take(a, K)):
        assert same(got, want[i])
    if src_pipe:
        wait_full(a)
    blob = a.state()
    assert a.state() == blob, "two gets with no batch delivered in between differ"
    # get does not disturb: the source goes on as the sampler that was never asked
    for i, got in enumerate(take(a, K)):
        assert same(got, want[K + i]), "get disturbed batch %d of its source" % (K + i)
    a.close()
    b = make(family)
    b.set_state(blob)
    if dst_pipe:
        b.prefetch_start(depth=DEPTH, threads=3)
    for i, got in enumerate(take(b, K)):
        assert same(got, want[K + i]), "resumed batch %d differs" % (K + i)
    b.close()


@pytest.mark.parametrize("family", ["window_fast", "general_q1"])
def test_state_is_the_consumers_not_the_pipelines(family):
    """The same position read from a serial and from a pipelined sampler (its ring full: three batches ahead) gives the same bytes."""
    a, b = make(family), make(family)
    b.prefetch_start(depth=DEPTH, threads=3)
    take(a, K), take(b, K)
    wait_full(b)
    assert a.state() == b.state()
    a.close(), b.close()


@pytest.mark.parametrize("family", ["window_fast", "general_q1", "negative_dataset"])
def test_refusals_leave_the_sampler_untouched(family):
    want = uninterrupted(family)
    a = make(family)
    take(a, K)
    blob = a.state()
    # late: after the first batch, and after prefetch_start
    with pytest.raises(VVError) as e:
        a.set_state(blob)
    assert e.value.code == VV_ERR_STATE
    assert same(a.next(want_last=True, want_label=True), want[K])
    a.close()
    c = make(family)
    c.prefetch_start(depth=DEPTH, threads=3)
    with pytest.raises(VVError) as e:
        c.set_state(blob)
    assert e.value.code == VV_ERR_STATE
    assert same(c.next(want_last=True, want_label=True), want[0])
    c.close()
    # other parameters
    o = make(family, batch_size=4)
    first = make(family, batch_size=4).next()
    with pytest.raises(VVError) as e:
        o.set_state(blob)
    assert e.value.code == VV_ERR_ARG and "batch_size" in str(e.value)
    assert np.array_equal(o.next(), first)
    o.close()
    # truncated, over-long, one fingerprint byte flipped (the fingerprint is bytes [24, 112) of the blob)
    b = make(family)
    flipped = bytearray(blob)
    flipped[40] ^= 0x04
    for bad in (blob[:-1], blob[:len(blob) // 2], blob[:100], blob[:8], b"", blob + b"\0", bytes(flipped)):
        with pytest.raises(VVError) as e:
            b.set_state(bad)
        assert e.value.code == VV_ERR_ARG, len(bad)
    assert same(b.next(want_last=True, want_label=True), want[0]), "a refused put changed the sampler"
    b.close()


def test_no_consumer_position():
    """A ring shared by two consumers, VV_SAMPLER_MODE=node, a stopped pipeline: VV_ERR_STATE."""
    s = make("window_fast")
    s.prefetch_start(depth=DEPTH, threads=3, consumers=2)
    with pytest.raises(VVError) as e:
        s.state()
    assert e.value.code == VV_ERR_STATE
    s.close()
    s = make("window_fast")
    s.prefetch_start(depth=DEPTH, threads=3)
    s.next()
    s.prefetch_stop()
    with pytest.raises(VVError) as e:
        s.state()
    assert e.value.code == VV_ERR_STATE
    s.close()
    s = make("window_fast")
    os.environ["VV_SAMPLER_MODE"] = "node"
    try:
        with pytest.raises(VVError) as e:
            s.state()
        assert e.value.code == VV_ERR_STATE
    finally:
        del os.environ["VV_SAMPLER_MODE"]
    s.state()
    s.close()


def test_plumbing():
    """The header prototypes, the library's exports, the binding and the facade's proto field 139."""
    hdr = open(os.path.join(ROOT, "include", "videovec.h")).read()
    for proto in ("int vv_sampler_state_size(vv_sampler* s, int64_t* bytes);",
                  "int vv_sampler_state_get(vv_sampler* s, void* buf, int64_t cap, int64_t* written);",
                  "int vv_sampler_state_put(vv_sampler* s, const void* buf, int64_t bytes);",
                  "int vv_run_state_size(vv_ctx* ctx, int64_t* bytes);",
                  "int vv_run_state_get(vv_ctx* ctx, void* buf, int64_t cap, int64_t* written);",
                  "int vv_run_state_put(vv_ctx* ctx, const void* buf, int64_t bytes);"):
        assert proto in hdr, proto
    for cite in ("solver.cpp:320-341, 578-596", "video_sampled_shots_data_layer.cpp:768-909"):
        assert cite in hdr, cite
    L = vv.load_library()
    for sym in ("vv_sampler_state_size", "vv_sampler_state_get", "vv_sampler_state_put",
                "vv_run_state_size", "vv_run_state_get", "vv_run_state_put"):
        assert isinstance(getattr(L, sym), C._CFuncPtr), sym
    for cls, names in ((vv.Sampler, ("state", "set_state")), (vv.Engine, ("run_state", "set_run_state"))):
        for n in names:
            assert callable(getattr(cls, n)), n
    src = open(os.path.join(ROOT, "caffe_facade", "src", "proto_lite.cpp")).read()
    assert re.search(r'OPTD\(139, "snapshot_data_state", T_BOOL, "false"\)', src), "SolverParameter.snapshot_data_state = 139 is not in the facade's schema"
