"""The whole option surface of vv_set_option / vv_get_option (include/videovec.h) on a fresh context: every name, its kind, its default,
and what each refusal says and leaves behind.  The surface stands here as literal data -- the defaults are those the library returned
on an MI355X before the two calls were rewritten over one table (csrc/api.hip: kOptions), not values read from the code under test --
so a name dropped from the table, or one that lost its read-only mark, fails here.

Needs no batch: vv_create alone, and for the three last_grad_* names also a context with parameters (D = F = 64; vv_params_set wants
the table's F first, so a 16-row synthetic table).  The environment's VV_* variables are removed: they set a context's initial values.
Setting "h16" after a forced fallback is tests/test_gpu_h16_guard.py's."""
import os

import pytest

pytestmark = pytest.mark.gpu

RT_MAX_K = 32            # csrc/vv_gallery_plan.h
W_CHUNKS_MAX = 4         # csrc/vv_internal.h

# name: (default, a valid value other than the default)
SETTABLE = {
    "dedup": (1, 0), "seg_bwd": (1, 0), "drop_dedup": (1, 2), "h16": (1, 0), "h16_guard": (1, 2), "slab16": (1, 0), "v16": (1, 0),
    "fuse_update": (1, 0), "fwd_lead": (1, 0), "wgrad_tr": (1, 0), "score_pf": (1, 0), "wgrad_lean": (1, 0), "comm_gate": (1, 0),
    "comm_inline": (1, 0), "wgrad_update": (1, 0), "comm_chunks": (3, 2), "comm_test_delay_us": (0, 5),
    "nearest_select_min_k": (33, 7), "cls_pass_tiles": (16384, 3), "cls_block_cols": (0, 64), "lin_split_rows": (0, 128),
}
# name: default
READ_ONLY = {
    "last_fwd_tile_rows": 0, "last_wgrad_splits": 0, "last_update_form": 0, "last_score_form": 0, "last_h16": 0,
    "last_grad_shift": 0, "last_grad_shift_round1": 0, "last_grad_repeat": 0,
    "h16_fallback": 0, "h16_flagged_step": -1, "h16_flagged_saturated": 0, "h16_flagged_faint_rows": 0,
    "last_cls_passes": 0, "last_cls_segments": 0, "last_cls_blocks": 0, "last_cls_row_ms": 0, "last_cls_count_ms": 0,
    "last_lin_splits": 0, "last_lin_blocks": 0, "last_lin_gather": 0, "last_lin_fwd_ms": 0, "last_lin_softmax_ms": 0,
    "last_lin_wgrad_ms": 0, "last_lin_update_ms": 0, "last_hinge_form": 0, "last_hinge_nonfinite": 0, "last_knn_form": 0,
}
RETIRED = ("fwd_merge", "score_stream", "comm_first_inline")
LAB = ("ablate", "lab_fwd_abl", "lab_wg_abl", "ph_mq")          # settable in a -DVV_LAB build only
# (name, refused value, how the message writes the value)
REFUSED = [
    ("drop_dedup", 3, "3"), ("h16_guard", 3, "3"), ("nearest_select_min_k", 0, "0"), ("nearest_select_min_k", RT_MAX_K + 2, str(RT_MAX_K + 2)),
    ("cls_pass_tiles", 0, "0"), ("cls_pass_tiles", 65536, "65536"), ("cls_block_cols", -1, "-1"), ("lin_split_rows", -1, "-1"),
]
ARG = r"videovec error 1: "                                   # VV_ERR_ARG, as Engine._chk writes it


@pytest.fixture
def eng(monkeypatch):
    import videovector_amd as vv
    for k in list(os.environ):
        if k.startswith("VV_") and k != "VV_LIB":
            monkeypatch.delenv(k)
    e = vv.Engine(0, "f16")
    yield e
    e.close()


def refused(eng, name, value, *words):
    import videovector_amd as vv
    with pytest.raises(vv.VVError) as ei:
        eng.set_option(name, value)
    msg = str(ei.value)
    assert msg.startswith(ARG) and ei.value.code == 1, msg
    for w in words:
        assert w in msg, (w, msg)


def test_surface_is_complete():
    assert len(SETTABLE) == 21 and len(READ_ONLY) == 27 and len(set(SETTABLE) | set(READ_ONLY) | set(RETIRED) | set(LAB)) == 21 + 27 + 3 + 4


def test_every_name_reads_its_default(eng):
    got = {n: eng.get_option(n) for n in list(SETTABLE) + list(READ_ONLY) + list(RETIRED)}
    print(got)
    want = {n: d for n, (d, _) in SETTABLE.items()}
    want.update(READ_ONLY)
    want.update({n: 0 for n in RETIRED})
    assert got == want


def test_last_grad_names_with_parameters(eng):
    import numpy as np
    eng.table_synth(7, 16, 64)
    eng.params_set(np.full((64, 64), 0.01, np.float32), np.zeros(64, np.float32))
    for n in ("last_grad_shift", "last_grad_shift_round1", "last_grad_repeat"):
        assert eng.get_option(n) == 0, n                        # no step yet
        refused(eng, n, 1, "read-only", n)


def test_read_only_names_refuse_every_set(eng):
    for n, d in READ_ONLY.items():
        for v in (0, 1):
            refused(eng, n, v, "read-only", n)
        assert eng.get_option(n) == d, n


def test_retired_names(eng):
    for n in RETIRED:
        assert eng.get_option(n) == 0
        eng.set_option(n, 0)
        refused(eng, n, 1, "retired", n)
        assert eng.get_option(n) == 0


def test_unknown_and_lab_names(eng):
    import videovector_amd as vv
    for n in ("no_such_option", "", "dedup ", "Dedup") + LAB:
        refused(eng, n, 0, "unknown option", "'%s'" % n)
        refused(eng, n, 1, "unknown option", "'%s'" % n)
        with pytest.raises(vv.VVError, match=ARG + r"vv_get_option: unknown option '%s'" % n):
            eng.get_option(n)


def test_settable_names_round_trip(eng):
    for n, (d, v) in SETTABLE.items():
        assert v != d, n
        eng.set_option(n, v)
        assert eng.get_option(n) == v, n
        for m, (dm, _) in SETTABLE.items():                     # ... and no other option moved
            if m != n:
                assert eng.get_option(m) == dm, (n, m)
        eng.set_option(n, d)
        assert eng.get_option(n) == d, n


@pytest.mark.parametrize("name,value,shown", REFUSED)
def test_range_refusals_leave_the_value(eng, name, value, shown):
    d, v = SETTABLE[name]
    for before in (d, v):
        eng.set_option(name, before)
        refused(eng, name, value, name + " = " + shown)
        assert eng.get_option(name) == before


def test_comm_chunks_clamps(eng):
    eng.set_option("comm_chunks", 0)
    assert eng.get_option("comm_chunks") == 1
    eng.set_option("comm_chunks", 99)
    assert eng.get_option("comm_chunks") == W_CHUNKS_MAX
