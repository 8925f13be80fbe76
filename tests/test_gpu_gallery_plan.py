"""The gallery's scratch from outside, through public getters only: after each call in a sequence on ONE gallery, scratch_bytes is the
call's block rows times the bytes of one row for the buffers that call needs (tests/gallery_plan_ref.py).  That fixes the sizes and the
drop-and-reallocate rule: a call that needs buffers the scratch lacks frees everything and allocates its own set, so a selection call
drops the class buffers and the other way round, and a call the scratch already serves leaves it alone.

300 items of dimension 20 with ids: Dp = 32, pitch = 320, one segment per row, 512-row query blocks."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gallery_plan_ref as ref   # noqa: E402

import videovector_amd as vv   # noqa: E402

pytestmark = pytest.mark.gpu
N, DIM = 300, 20


def test_scratch_follows_the_plan_call_by_call():
    rng = np.random.default_rng(7)
    feat = rng.standard_normal((N, DIM)).astype(np.float32)
    ids = (np.arange(N) // 3).astype(np.int32)
    sh = ref.shape(N, DIM)
    assert (sh["Dp"], sh["pitch"], sh["S"], sh["qb_max"]) == (32, 320, 1, 512)
    eng = vv.Engine(0, "f16")
    g = eng.gallery(feat, ids)
    try:
        assert g.scratch_bytes == 0 and g.get("query_block") == sh["qb_max"]

        def check(rows, cls, sel):
            assert g.scratch_bytes == rows * ref.row_bytes(sh, cls, sel), (g.scratch_bytes, rows, cls, sel)
            assert g.get("query_block") == sh["qb_max"]

        q = feat[:7] + 0.01
        g.topk(q, 3)                                             # 1. seven rows, the plain set
        check(7, False, False)
        assert 40 >= eng.get_option("nearest_select_min_k")
        g.nearest(q, 40)                                         # 2. the selection form: everything dropped, seven rows with its buffers
        assert g.get("last_nearest_form") == 2
        check(7, False, True)
        g.class_stats({int(i): int(i) % 5 for i in np.unique(ids)})     # 3. every item a query: 300 rows, the class buffers, no selection buffers
        check(N, True, False)
        g.nearest(q, 5)                                          # 4. the streaming form: the scratch at hand serves it
        assert g.get("last_nearest_form") == 1
        check(N, True, False)
    finally:
        g.close()
        eng.close()
