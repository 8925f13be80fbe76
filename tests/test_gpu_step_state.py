"""Every call that may follow a backward pass, from every place the gradient can be (videovector_amd/csrc/vv_step_state.h: GradAt).

Two engines with the same seed run the same calls: one with fuse_update = 0 -- it reduces at the end of every backward pass, so its
gradient is always in the buffer: the eager reference -- and one with the defaults, which keeps the gradient in the split-K slabs and, at
one split of K with vv_update_hint, updates W in the weight-gradient GEMM.  For each place the default engine's gradient can be in on one
rank (None, Slabs, SlabsStale, Buffer; SlabsWUpdated and Lost at the one-split shape) and each call (loss, grads, grads_device,
apply_update, apply_update twice, params_set followed by a step, vv_op_inner_product_bwd followed by grads), over three steps, the call
returns the eager engine's result bit for bit (np.array_equal) -- or the VVError that include/videovec.h documents for a step announced by
vv_update_hint: exactly in the (place, call) pairs of REFUSED below, nowhere else.  Parameters, histories and the loss after the three
steps are bit-equal too.

After vv_op_inner_product_bwd the gradient read back is that operator's, not the step's: X and dY are uniform in [0, 1), so dW = dY^T X has
no cancellation and every element is within 2^-10 of the float64 product, relatively (each operand rounded once to f16, 2^-11 each; the
scales are powers of two; fp32 accumulation over R = 64 rows adds 64 x 2^-24); db is the fp32 column sum of dY (64 x 2^-24).  The bound
asserted is 2^-9 on dW and 2^-17 on db, element by element.

The one-split shape: B 128, C 5, Nn 10 with D = F = 3844 -- the weight-gradient GEMM has one split of K when its 256 x 256 tiles number
at least 256, i.e. from a padded 4096 x 4096 on: D in 3841 .. 4096, and the lazy reduction wants F % 4 == 0.  The test asserts
last_update_form == 5 there (and 3 or 4 at the small shape), so a shape that stops qualifying fails and does not pass vacuously.
"""
import numpy as np
import pytest

from tests.test_gpu_parity import vv  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

PLACES = ["None", "Slabs", "SlabsStale", "Buffer"]
HINTED = ["SlabsWUpdated", "Lost"]
CALLS = ["loss", "grads", "grads_device", "apply_update", "apply_update_twice", "params_set_step", "ip_bwd_grads"]
# the documented refusals (include/videovec.h, vv_update_hint): between a hinted, fused backward pass and its update only vv_loss_get and
# vv_apply_update; after it the gradient was never stored
REFUSED = {("SlabsWUpdated", "grads"), ("SlabsWUpdated", "grads_device"), ("SlabsWUpdated", "ip_bwd_grads"),
           ("Lost", "grads"), ("Lost", "grads_device"), ("Lost", "apply_update"), ("Lost", "apply_update_twice")}
R_OP = 64


class Pair:
    """The eager engine, the default one, and what both are fed."""

    def __init__(self, vv, B, C, Nn, F, D, n_videos):  # noqa: F811
        from videovector_amd.synth import SyntheticVideos, init_weights
        self.vv, self.shape = vv, (B, C, Nn, F, D)
        ds = SyntheticVideos(seed=1701, n_videos=n_videos)
        smp = vv.Sampler(ds.video_id, ds.n_shots, ds.row_base, batch_size=B, context_size=C, num_negative_samples=Nn,
                         max_buffer_size=500, negative_swap_percentage=50)
        self.idx = [np.ascontiguousarray(smp.next()) for _ in range(4)]
        smp.close()
        self.ds = ds
        self.W, self.b = init_weights(1, D, F, std=0.02)
        self.cfg = vv.StepConfig(B, C, Nn, lr=0.01, momentum=0.9, weight_decay=5e-4)
        rng = np.random.default_rng(5)
        self.X = rng.random((R_OP, F), dtype=np.float32)
        self.dY = rng.random((R_OP, D), dtype=np.float32)
        self.dW_op = self.dY.astype(np.float64).T @ self.X.astype(np.float64)
        self.db_op = self.dY.astype(np.float64).sum(0)
        self.eng = None

    def engines(self):
        """(eager, default), with fresh parameters and no gradient: vv_params_set starts every scenario."""
        if self.eng is None:
            self.eng = []
            for fuse in (0, 1):
                e = self.vv.Engine(0, "f16")
                if not fuse:
                    e.set_option("fuse_update", 0)
                e.table_synth(self.ds.seed, self.ds.n_rows, self.shape[3])
                e.params_set(self.W, self.b)
                e.Xd, e.Yd, e.dYd = e.dev(self.X), e.dev((R_OP, self.shape[4])), e.dev(self.dY)
                e.op("inner_product", e.Xd, R_OP, e.Yd)          # (vv_op_inner_product_bwd reuses its 16-bit copy of X)
                self.eng.append(e)
        for e in self.eng:
            e.params_set(self.W, self.b)
        return self.eng

    def drop(self):
        """New engines for the next scenario (vv_grads_device succeeded: the reduction is eager from then on)."""
        for e in self.eng or []:
            e.close()
        self.eng = None


def call(pair, eng, name, k, second=None):
    """One call of CALLS on one engine: (its value, whether this step's update is now applied).  VVError propagates.
    second: apply_update_twice's second update -- None: try it (it is refused where the first one finished a step whose gradient was never
    stored), True / False: make it or not, as the other engine did."""
    cfg = pair.cfg
    if name == "loss":
        return eng.loss(), False
    if name == "grads":
        return eng.grads(), False
    if name == "grads_device":
        ptr, n = eng.grads_device()
        assert ptr and n == pair.shape[4] * pair.shape[3] + pair.shape[4]
        return eng.grads(), False                                # (what the holder of the pointer reads: the flat buffer)
    if name == "apply_update":
        eng.apply_update(cfg)
        return eng.loss(), True
    if name == "apply_update_twice":
        eng.apply_update(cfg)
        try:
            if second is not False:
                eng.apply_update(cfg)
            second = second is not False
        except pair.vv.VVError as e:
            assert second is None and "never stored" in str(e), str(e)
            second = False
        return (eng.loss(), second), True
    if name == "params_set_step":
        eng.params_set(pair.W, pair.b)
        eng.forward_backward(cfg, pair.idx[3])
        eng.apply_update(cfg)
        return eng.loss(), True
    assert name == "ip_bwd_grads"
    eng.op("inner_product_bwd", eng.dYd, R_OP, 0.0)
    return eng.grads(), False


def outcome(pair, eng, name, k, second=None):
    try:
        return call(pair, eng, name, k, second)
    except pair.vv.VVError as e:
        return ("VVError", str(e)), None


def same(a, b):
    if isinstance(a, tuple) and isinstance(b, tuple):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, str) or isinstance(b, str):
        return isinstance(a, str) and isinstance(b, str)         # (two refusals: the messages name different reasons at most)
    return np.array_equal(np.asarray(a), np.asarray(b))


def run(pair, place, name, forms):
    eager, lazy = pair.engines()
    cfg, what = pair.cfg, "%s / %s" % (place, name)
    hinted = place in HINTED
    for k in range(3):
        updated = False
        if place != "None" or k > 0:                             # ("None": the call comes before the first backward pass, then whole steps)
            for e in (eager, lazy):
                if hinted:
                    e.update_hint(cfg)
                e.forward_backward(cfg, pair.idx[k])
                if place in ("SlabsStale", "Lost"):
                    e.apply_update(cfg)
                if place == "Buffer":
                    e.loss()                                     # (a reader: the default engine reduces now)
            updated = place in ("SlabsStale", "Lost")
        if place == "None" and k > 0:
            for e in (eager, lazy):
                e.apply_update(cfg)
            continue
        got, done = outcome(pair, lazy, name, k)
        refused = isinstance(got[0], str) and got[0] == "VVError"
        assert refused == ((place, name) in REFUSED) or place == "None", "%s, step %d: %r" % (what, k, got if refused else "no VVError")
        if refused and place != "None":
            assert "vv_update_hint" in got[1], got[1]            # the documented refusal, not some other failure
        else:
            if name == "apply_update_twice" and not refused:
                assert got[1] == (place != "SlabsWUpdated"), what   # (the first update finished the hinted step: -> Lost)
            want, done_e = outcome(pair, eager, name, k, got[1] if name == "apply_update_twice" and not refused else None)
            assert same(got, want), "%s, step %d: differs from the eager engine" % (what, k)
            assert done == done_e
            if name == "ip_bwd_grads" and not refused:
                dW, db = got
                assert np.all(np.abs(dW - pair.dW_op) <= 2.0 ** -9 * pair.dW_op), what + ": dW is not the operator's"
                assert np.all(np.abs(db - pair.db_op) <= 2.0 ** -17 * pair.db_op), what + ": db is not the operator's"
        for e in (eager, lazy):
            if place != "None" and not updated and not (done and not refused):
                e.apply_update(cfg)
        forms.add(int(lazy.get_option("last_update_form")))
    for a, b, n in zip(eager.params_get(), lazy.params_get(), ("W", "b", "hW", "hb")):
        assert np.array_equal(a, b), "%s: %s differs from the eager engine after three steps" % (what, n)
    if place != "None" or name == "params_set_step":
        assert eager.loss() == lazy.loss(), what
    if name == "grads_device" and place not in HINTED:
        pair.drop()


def test_every_call_from_every_place_small(vv):  # noqa: F811
    """B 32, C 5, Nn 2, F 128, D 32 (the smoke shape): several splits of K, so None, Slabs, SlabsStale and Buffer."""
    pair = Pair(vv, 32, 5, 2, 128, 32, 50)
    forms = set()
    for place in PLACES:
        for name in CALLS:
            run(pair, place, name, forms)
    pair.drop()
    assert forms & {3, 4}, forms                                 # the fused reduce + update ran (lazy reduction)
    assert 5 not in forms, forms


def test_every_call_from_every_place_one_split(vv):  # noqa: F811
    """B 128, C 5, Nn 10, D = F = 3844: one split of K, the hinted step updates W in the weight-gradient GEMM (SlabsWUpdated, Lost)."""
    pair = Pair(vv, 128, 5, 10, 3844, 3844, 512)
    forms = set()
    for place in HINTED:
        for name in CALLS:
            run(pair, place, name, forms)
    pair.drop()
    assert 5 in forms, forms
