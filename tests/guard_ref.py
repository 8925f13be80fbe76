"""The f16 gradient-scale guard's protocol, restated in numpy float64 from its documentation (tests only; reads no engine code).

The 16-bit gradient rows carry one power-of-two scale per step: the host's sg times 2^-shift, the shift chosen on the device.

Per-instance rows, one round (dense execution).  Round 0 writes the rows dY sg and records M0 = max |dY sg|.  The repeat is active iff
M0 > 32768; then shift = max(e - 12, 1) with M0 = f 2^e, f in [0.5, 1): the largest value comes to lie in [2^11, 2^12).

Rows plus their segment sums, two rounds (de-duplicated execution without the segment-wise backward).  Round 0 records the rows' true
maximum and the maximum of the sums formed FROM THE ROWS AS STORED: rounded to f16, saturated at +-65504; summed in double.  Round 1 is
active iff either passes 32768, its shift comes from the larger.  Round 2 is active iff one of round 1's maxima (rows and sums of the rows
as round 1 stored them, at sg 2^-shift1) passes 32768; its shift adds to round 1's.  Sums of clipped rows under-report: that is what round 2
is for.

Host steering.  The step with sequence number seq runs at sg = 2^(e + sg_adj), e the exponent of the loss count (count = f 2^e).  Until
seq - seq0 >= lag (4) nothing moves; then the report (gmax, repeat bit) of step seq - lag is read -- gmax the step's round-0 maximum over
its sg -- and ex = exponent(gmax) + e + sg_adj; ex > 13 or ex < 5: sg_adj += 10 - ex.  Every step clamps sg_adj to [-100 - e, 100 - e].
`repeats` counts the reports read with the repeat bit set.

Every decision comes back with its distance from its threshold (`decisions`: name, value, threshold), and `margin_ok` says whether each
value is at least a factor 1 +- 2^-10 away: the fp32 maxima of the kernels differ from these float64 ones by about 1e-6, so a case that
passes `margin_ok` has one answer.  A case that does not is no case: move the seed or the magnitude.

The keyword arguments `place`, `clip` and `lag` exist for tests/test_guard_ref_host.py, which shows that a changed rule changes the answer.
"""
import numpy as np

LIMIT = 32768.0
F16_MAX = 65504.0
MARGIN = 2.0 ** -10


def exponent(x):
    """e with x = f 2^e, f in [0.5, 1)"""
    return int(np.frexp(np.float64(x))[1])


def f16_stored(x):
    """float64 -> what an f16 row holds (round to nearest even, saturated at +-65504), as float64"""
    return np.clip(np.asarray(x, np.float64), -F16_MAX, F16_MAX).astype(np.float16).astype(np.float64)


def _pow2_decision(name, v):
    """the two power-of-two boundaries around v > 0"""
    e = exponent(v)
    return [(name + " vs 2^%d" % (e - 1), v, 2.0 ** (e - 1)), (name + " vs 2^%d" % e, v, 2.0 ** e)]


def margin_ok(decisions, margin=MARGIN):
    """(ok, worst): every (name, value, threshold) has value >= threshold (1 + margin) or value <= threshold (1 - margin); worst: the
    decision nearest its threshold as (name, value / threshold)"""
    ok, worst, best = True, ("none", np.inf), np.inf
    for name, v, t in decisions:
        assert v > 0 and t > 0
        r = v / t
        if not (r >= 1 + margin or r <= 1 - margin):
            ok = False
        if abs(np.log2(r)) < best:
            best, worst = abs(np.log2(r)), (name, r)
    return ok, worst


def _shift_from(m, place):
    return max(exponent(m) - place, 1)


def guard_rounds(dY, sg, path, seg_map=None, place=12, clip=True):
    """dY [R][D] float64 per-instance gradient rows (unscaled), sg the host's scale (a power of two), path "dense" (one round) or "sum"
    (two rounds; seg_map [R]: the slot of every instance).  Returns a dict:
      rounds        per guard round r = 1 ..: dict(active, shift (cumulative, from this round on), rows_max, sums_max -- the maxima of the round
                    BEFORE it, which decided it, in that round's scaled units)
      shift         the step's final shift;  shift_round1;  repeat (a conditional repeat really ran);  scale = sg 2^-shift
      gmax          what the step reports: its round-0 maximum over sg
      decisions     [(name, value, threshold)]: see margin_ok"""
    dY = np.asarray(dY, np.float64)
    assert path in ("dense", "sum") and np.frexp(sg)[0] == 0.5
    n_rounds = 1 if path == "dense" else 2
    m = None
    if path == "sum":
        m = np.asarray(seg_map, np.int64)
        assert m.shape == (dY.shape[0],)

    def maxima(shift):
        rows = dY * (sg * 2.0 ** -shift)
        rm = float(np.abs(rows).max())
        sm = 0.0
        if m is not None:
            sums = np.zeros((int(m.max()) + 1, dY.shape[1]))
            np.add.at(sums, m, f16_stored(rows) if clip else rows)
            sm = float(np.abs(sums).max())
        return rm, sm

    decisions, rounds = [], []
    shift = 0
    rm, sm = maxima(0)
    gmax = max(rm, sm) / sg
    for r in range(1, n_rounds + 1):
        for name, v in (("round %d rows" % (r - 1), rm), ("round %d sums" % (r - 1), sm)):
            if v > 0:
                decisions.append((name + " vs the limit", v, LIMIT))
        active = max(rm, sm) > LIMIT
        if active:
            big = max(rm, sm)
            decisions += _pow2_decision("round %d maximum" % (r - 1), big)
            shift += _shift_from(big, place)
        rounds.append(dict(active=active, shift=shift, rows_max=rm, sums_max=sm))
        if r < n_rounds:
            rm, sm = maxima(shift)
    return dict(rounds=rounds, shift=shift, shift_round1=rounds[0]["shift"], repeat=int(any(q["active"] for q in rounds)),
                scale=sg * 2.0 ** -shift, gmax=gmax, decisions=decisions)


class Steering:
    """The host's side.  begin(seq) -> the step's sg, after reading the report due; report(seq, gmax, repeat_bit) files a step's report
    (a step whose reduction never ran files none).  count: the loss count B Nn (or global_count)."""

    def __init__(self, count, lag=4):
        self.e = exponent(count)
        self.lag = lag
        self.sg_adj = 0
        self.repeats = 0
        self.seq0 = None
        self.reports = {}
        self.decisions = []

    def begin(self, seq):
        if self.seq0 is None:
            self.seq0 = seq
        if seq - self.seq0 >= self.lag and seq - self.lag in self.reports:
            gmax, bit = self.reports[seq - self.lag]
            if bit:
                self.repeats += 1
            if gmax > 0 and np.isfinite(gmax):
                v = float(gmax) * 2.0 ** (self.e + self.sg_adj)
                self.decisions += _pow2_decision("step %d: report of step %d" % (seq, seq - self.lag), v)
                ex = exponent(gmax) + self.e + self.sg_adj
                if ex > 13 or ex < 5:
                    self.sg_adj += 10 - ex
        self.sg_adj = max(-100 - self.e, min(100 - self.e, self.sg_adj))
        return 2.0 ** (self.e + self.sg_adj)

    def report(self, seq, gmax, repeat_bit):
        self.reports[seq] = (float(gmax), int(bool(repeat_bit)))


def steering_run(dY, count, path, steps, seg_map=None, lag=4, first_seq=1):
    """The same gradient rows for `steps` steps: per step dict(sg, repeats (as the host counts them after issuing the step), + guard_rounds'
    fields).  decisions of every step and of the steering are gathered in the last element's "all_decisions"."""
    st = Steering(count, lag)
    out, dec, cache = [], [], {}
    for i in range(steps):
        seq = first_seq + i
        sg = st.begin(seq)
        if sg not in cache:
            cache[sg] = guard_rounds(dY, sg, path, seg_map)
        g = dict(cache[sg])
        st.report(seq, g["gmax"], g["repeat"])
        g.update(sg=sg, repeats=st.repeats)
        dec += g["decisions"]
        out.append(g)
    out[-1]["all_decisions"] = dec + st.decisions
    return out
