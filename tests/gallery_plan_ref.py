"""The gallery scratch's sizing arithmetic restated in Python from the entry points as they stood before videovector_amd/csrc/
vv_gallery_plan.h existed (gallery_init, gallery_ensure_scratch, gallery_nearest_run, vv_gallery_class_stats, each with a sum of its
own): what the header's functions are compared with, on the host (test_gallery_plan_host.py) and from outside on the device
(test_gpu_gallery_plan.py)."""

SCRATCH_MAX = 1 << 30                   # every device buffer a query call needs, together
DIST_MAX = SCRATCH_MAX - (40 << 20)     # ... of which the distances
QB_MAX = 512                            # rows of one query block at most
SEG_MAX = 64                            # gallery segments (workgroups) per row at most
BK, CHUNK, MAX_K, SEL_BINS, SEL_LAST_BINS = 32, 2048, 32, 4096, 256
ACC = 24                                # RankAcc / ClassAcc: a double and four int32


def _round_up(x, a):
    return (x + a - 1) // a * a


def shape(n_ref, dim):
    """gallery_init: dict(Dp, pitch, seg, S, qb_max); qb_max 0 is its 'do not fit one query row' error."""
    pitch = _round_up(n_ref, 64)
    seg = max(_round_up((n_ref + SEG_MAX - 1) // SEG_MAX, 1024), 16384)
    return dict(Dp=_round_up(dim, BK), pitch=pitch, seg=seg, S=(n_ref + seg - 1) // seg, qb_max=min(QB_MAX, DIST_MAX // (pitch * 4)))


def row_bytes(sh, cls, sel):
    """gallery_ensure_scratch's total for one row: b_dist + b_q + b_part + b_bins + 2 b_out + 3 b_row + b_acc, the class pair
    (skeys + cbins), the selection form's buffers and -- without the class pair -- the skeys it shares."""
    b = sh["pitch"] * 4 + sh["Dp"] * 4 + sh["S"] * MAX_K * 8 + 2 * CHUNK * 4 + 2 * (MAX_K * 4) + 3 * 4 + ACC
    class_row = CHUNK * 8 + 3 * CHUNK * 4
    sel_row = 4 * 4 + SEL_BINS * 4 + sh["S"] * SEL_LAST_BINS * 4 + 2 * CHUNK * 4
    if cls:
        b += class_row
    if sel:
        b += sel_row + (0 if cls else CHUNK * 8)
    return b


def block_rows(sh, n_q, cls, sel):
    """Rows of a call's blocks.  gallery_call_begin (no flag): min(n_q, qb_max), no division.  gallery_nearest_run's selection form and
    vv_gallery_class_stats: that, and the scratch limit over their own row sum; 0 is their 'do not fit one query row' error."""
    block = min(n_q, sh["qb_max"])
    if cls or sel:
        block = min(block, SCRATCH_MAX // row_bytes(sh, cls, sel))
    return block
