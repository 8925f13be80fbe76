"""The backward half's host decisions (videovector_amd/csrc/vv_backward_plan.h) restated from the rules in words -- the comments of the step
and DESIGN.md 3.5 / 3.6 / 8 -- for tests/test_backward_plan_host.py (every case of the check tool) and tests/test_gpu_backward_plan.py (what
a real step must report).  Nothing here is read from the library."""
from fractions import Fraction

BM = BN = 256          # the weight-gradient GEMM's output tile
BK = 64                # one K-step: 64 batch rows (and one K-tile of the forward GEMM: 64 features)
WMAX_SLOTS = 2048      # per-block maxima one buffer holds
SGD_BLOCKS = 1024      # k_sgd's grid
SEGB_BLOCKS = 1024     # k_seg_bwd's grid
CUS = 256


def pad(v, a=256):
    return -(-v // a) * a


def split_k(Dp, Fp, Rp):
    """About one wave of workgroups over the chip's 256 CUs: each of the (Dp / 256) (Fp / 256) output tiles is cut along K into as many
    splits as it takes to reach 256 workgroups -- but a split is at least one K-step of 64 rows, and there is at least one split.  The
    K-steps are dealt out evenly, rounded up."""
    tiles = (Dp // BM) * (Fp // BN)
    steps = Rp // BK
    S = max(1, min(-(-CUS // tiles), steps))
    return S, -(-steps // S)


def chunks(nk, n_chunks):
    """F-chunks of the overlapped update over nk K-tiles: at most n_chunks and at most one per 8 K-tiles, widths in the ratio 1 : 0.6 :
    0.36 : ..., every inner boundary rounded to the nearest K-tile and then down to an even one; a boundary must lie at least 4 tiles
    behind the one before and at least 4 before the end, else one chunk fewer is tried.  Returns the boundaries [0, ..., nk]."""
    n = max(1, min(n_chunks, nk // 8))
    while True:
        w = [Fraction(3, 5) ** i for i in range(n)]
        kt = [0]
        for i in range(1, n):
            exact = nk * sum(w[:i]) / sum(w)
            kt.append(int(exact + Fraction(1, 2)) // 2 * 2)
        kt.append(nk)
        inner_ok = all(kt[i] >= kt[i - 1] + 4 and kt[i] <= nk - 4 for i in range(1, n))
        if inner_ok or n == 1:
            return kt
        n -= 1


def backward(i, wmax_slots=WMAX_SLOTS):
    """i: the inputs by the names the check tool prints (world 0: no communicator).  Returns the outputs by the names it prints.

    Where the gradient goes.  With a communicator the exchange decides: the sharded schedule lays the buffer out shard-major, the overlapped
    one chunk-major -- both only in the library's own buffer that nobody was handed (a bound buffer, or a holder of vv_grads_device's
    pointer, reads the documented flat layout) and only with 16-byte groups of floats (F % 4 = 0); sharded further needs D to split into
    `world` equal shards of whole 4-row groups and every rank's share of the SGD grid's per-block maxima to fit one buffer; sharded wins
    over overlapped.  Without a communicator the gradient can stay in the split-K slabs until somebody wants it (option fuse_update),
    under the same buffer conditions, F % 4 = 0 and at most 8 slabs.  Otherwise k_reduce writes it out flat at once."""
    world = i["world"]
    has_comm = world > 0
    private_buffer = bool(i["grads_own"]) and not i["grads_exposed"]
    vec4 = i["F"] % 4 == 0
    o = {"shard_rows": i["D"] // world if has_comm else 0}
    even_shards = has_comm and o["shard_rows"] * world == i["D"] and o["shard_rows"] % 4 == 0
    maxima_fit = has_comm and world * (SGD_BLOCKS // world) <= wmax_slots
    o["sharded"] = has_comm and bool(i["comm_sharded"]) and private_buffer and vec4 and even_shards and maxima_fit
    o["chunked"] = has_comm and bool(i["comm_overlap"]) and private_buffer and vec4 and not o["sharded"]
    o["lazy"] = not has_comm and bool(i["fuse_update"]) and private_buffer and vec4 and i["S"] <= 8
    # The update in the weight-gradient GEMM's epilogue: a step announced by vv_update_hint whose gradient would stay in the slabs, with
    # ONE split of K (the accumulator tile is the gradient), in the phase-staggered kernel, option wgrad_update on, one per-block maximum
    # per tile fitting the buffer; not for Adam (two histories), not under clipping (needs the whole norm first), not when the lab asks
    # for the gradient to be kept
    tiles = (i["Dp"] // BM) * (i["Fp"] // BN)
    declined = bool(i["hint_adam"]) or bool(i["hint_clip"]) or bool(i["fuse_keep_grads"])
    o["fuse_w"] = (bool(i["hinted"]) and bool(i["wgrad_update"]) and bool(i["can_fuse_update"]) and o["lazy"] and i["S"] == 1
                   and tiles <= wmax_slots and not declined)
    # f16 split-K partial products: several splits (2 .. 8) of the phase-staggered kernel, 16-byte groups of f16 (F % 8 = 0); with one
    # split there is nothing to sum
    o["slab16"] = bool(i["slab16"]) and bool(i["can_fuse_update"]) and 2 <= i["S"] <= 8 and i["F"] % 8 == 0 and not o["fuse_w"]
    # the lean weight-gradient loop addresses the table with 24-bit row ids, 24-bit byte offsets inside a row of 16-bit values, and 32-bit
    # byte offsets overall, one 8 KiB K-tile of slack included
    rows, row_bytes = i["table_rows"], i["Fp"] * 2
    o["lean"] = bool(i["wgrad_lean"]) and rows < 2 ** 24 and row_bytes < 2 ** 24 and rows * row_bytes + 8192 < 2 ** 32
    # The f16 gradient-scale guard.  bf16: none.  The segment-wise pair settles the scale on the device before it rounds (proactive: no
    # repeat); the lab can switch that off, which leaves one repeat as for per-instance rows; de-duplicated without the pair rounds twice
    # (the rows, then their sums): two repeats.  Who reports maxima: the pair's k_seg_bwd grid alone; else the score kernel's B items,
    # and k_segsum over groups of 4 padded rows when de-duplicated.
    o["proactive"] = bool(i["seg"]) and bool(i["guard_proactive"])
    if not i["f16"] or o["proactive"]:
        o["n_rounds"] = 0
    else:
        o["n_rounds"] = 2 if (i["dd"] and not i["seg"]) else 1
    if i["seg"]:
        o["n_of0"], o["n_of1"] = 0, SEGB_BLOCKS
    else:
        o["n_of0"], o["n_of1"] = i["B"], (-(-i["Rp"] // 4) if i["dd"] else 0)
    return {k: int(v) for k, v in o.items()}


def update_form(plan, F):
    """Option "last_update_form" after vv_apply_update of a step without a communicator, clipping or a bank: the slabs reduced and
    updated in one launch (3, with f16 slabs 4; 5 when the weight-gradient GEMM updated the matrix itself), else k_sgd on the flat
    buffer, 16 bytes at a time (1) or element-wise (2)."""
    if plan["fuse_w"]:
        return 5
    if plan["lazy"]:
        return 4 if plan["slab16"] else 3
    return 1 if F % 4 == 0 else 2
