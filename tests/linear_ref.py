"""Restatement of the softmax linear classifier (include/videovec.h, vv_linear_*) in numpy: one step and a fit -- the batches,
the cursor, the rule -- in float64, and beside it a float32 twin that rounds where the device rounds (the sums' orders differ in the
two products only).  softmax_layer.cpp:25-59, softmax_loss_layer.cpp:34-83, inner_product_layer.cu:12-59, solver.cpp:485-531."""
import numpy as np

FLT_MIN = np.float32(1.17549435e-38)
EPS = 2.0 ** -23          # one ulp of a float in [1, 2), the relative size of an ulp at most
F32 = np.float32


def first_max(z):
    """The lowest column attaining the maximum over the non-NaN logits of each row; 0 where there is none."""
    z = np.asarray(z)
    return np.argmax(np.where(np.isnan(z), -np.inf, z), axis=1)


def lanes_of(cols):
    """Lanes that share one row in k_softmax_xent: 32 (two rows per wave) up to 32 columns, else 64."""
    return 32 if cols <= 32 else 64


def rows_per_pass(cols):
    """Rows one pass of k_softmax_xent's fixed grid covers: 512 workgroups x 4 waves x rows per wave."""
    return 512 * 4 * (64 // lanes_of(cols))


def softmax_loss(z, labels, loss_weight=1.0):
    """float64: (p, dz, loss, correct) of logits z [rows][cols]."""
    z = np.asarray(z, np.float64)
    rows = z.shape[0]
    idx = np.arange(rows)
    m = z[idx, first_max(z)][:, None]
    e = np.exp(z - m)
    p = e / e.sum(axis=1, keepdims=True)
    terms = -np.log(np.maximum(p[idx, labels], np.float64(FLT_MIN)))
    onehot = np.zeros_like(p)
    onehot[idx, labels] = 1.0
    dz = (p - onehot) * (loss_weight / rows)
    return p, dz, loss_weight * terms.sum() / rows, int((first_max(z) == labels).sum())


def softmax_loss_f32(z, labels, loss_weight=1.0):
    """The float32 twin: the subtraction, exp, the row sum lane-strided ascending then folded by halves, the division, the scale
    loss_weight / rows formed once in fp32; the loss terms in fp32, their sum in double."""
    z = np.asarray(z, F32)
    rows, cols = z.shape
    idx = np.arange(rows)
    wd = lanes_of(cols)
    m = z[idx, first_max(z)][:, None]
    e = np.exp(z - m, dtype=F32)
    chunks = -(-cols // wd)
    ep = np.zeros((rows, chunks * wd), F32)
    ep[:, :cols] = e
    ep = ep.reshape(rows, chunks, wd)
    part = np.zeros((rows, wd), F32)
    for k in range(chunks):
        part = part + ep[:, k, :]
    o = wd // 2
    while o > 0:
        part = part[:, :o] + part[:, o:2 * o]
        o //= 2
    p = e / part
    scale = F32(loss_weight) / F32(rows)
    onehot = np.zeros_like(p)
    onehot[idx, labels] = 1
    dz = ((p - onehot) * scale).astype(F32)
    terms = -np.log(np.maximum(p[idx, labels], FLT_MIN), dtype=F32)
    loss = F32(np.float64(F32(loss_weight)) * terms.astype(np.float64).sum() / rows)
    return p, dz, loss, int((first_max(z) == labels).sum())


def batches(n, batch, iters, cursor=0):
    """[(first, count)] of `iters` steps and the cursor afterwards: batch 0 is the whole set; otherwise consecutive items from the
    cursor, a batch never wraps, the cursor returns to 0 behind the last batch of an epoch."""
    b = n if batch == 0 else min(batch, n)
    out = []
    for _ in range(iters):
        count = min(b, n - cursor)
        out.append((cursor, count))
        cursor += count
        if cursor >= n:
            cursor = 0
    return out, cursor


class State:
    """W [C][dim], b [C], their histories, the step counter and the cursor."""

    def __init__(self, dim, C, dtype=np.float64, bias=True):
        self.W, self.hW = np.zeros((C, dim), dtype), np.zeros((C, dim), dtype)
        self.b, self.hb = np.zeros(C, dtype), np.zeros(C, dtype)
        self.bias, self.dtype, self.steps, self.cursor = bias, dtype, 0, 0


def gradient(st, X, y, loss_weight=1.0):
    """(dW, db, loss, correct) of one batch at st's parameters, in st's dtype."""
    if st.dtype == np.float64:
        X = np.asarray(X, np.float64)
        z = X @ st.W.T + (st.b if st.bias else 0.0)
        _, dz, loss, correct = softmax_loss(z, y, loss_weight)
    else:
        X = np.asarray(X, F32)
        z = (X @ st.W.T).astype(F32)
        if st.bias:
            z = z + st.b
        _, dz, loss, correct = softmax_loss_f32(z, y, loss_weight)
    dW = (dz.T @ X).astype(st.dtype)
    db = dz.sum(axis=0).astype(st.dtype) if st.bias else np.zeros_like(st.b)
    return dW, db, loss, correct


def step(st, X, y, lr, momentum, weight_decay, loss_weight=1.0):
    """h = lr (g + weight_decay W) + momentum h; W -= h -- every product and sum rounded as written in st's dtype; no decay on b."""
    t = st.dtype
    dW, db, loss, correct = gradient(st, X, y, loss_weight)
    lr, momentum, weight_decay = t(lr), t(momentum), t(weight_decay)
    st.hW = lr * (dW + weight_decay * st.W) + momentum * st.hW
    st.W = st.W - st.hW
    if st.bias:
        st.hb = lr * db + momentum * st.hb
        st.b = st.b - st.hb
    st.steps += 1
    return loss, correct


def fit(st, X, y, iters, batch=0, lr=0.1, momentum=0.9, weight_decay=0.0, loss_weight=1.0, lr_schedule=None):
    """(loss trace, accuracy of the last batch); st.cursor is carried."""
    y = np.asarray(y)
    plan, cursor = batches(len(X), batch, iters, st.cursor)
    trace, acc = [], 0.0
    for t, (first, count) in enumerate(plan):
        rate = lr if lr_schedule is None else lr_schedule[t]
        loss, correct = step(st, X[first:first + count], y[first:first + count], rate, momentum, weight_decay, loss_weight)
        trace.append(loss)
        acc = correct / count
    st.cursor = cursor
    return np.array(trace), acc


def blobs(n=256, C=4, dim=8, seed=7):
    """The blob inputs: label i % C, class mean 3 e_c, noise 0.5 N(0, 1) from RandomState(seed), rounded to fp32."""
    rs = np.random.RandomState(seed)
    y = (np.arange(n) % C).astype(np.int32)
    X = 0.5 * rs.randn(n, dim)
    X[np.arange(n), y] += 3.0
    return X.astype(F32), y


def p_bound(cols, spread):
    """Relative bound on the device's p against float64 from the same fp32 logits, in units of 1 (not ulps); see
    tests/test_gpu_softmax_exact.py's docstring for the count."""
    wd = lanes_of(cols)
    depth = -(-cols // wd) + int(np.log2(wd))
    ulps = 2 * (3 + spread / 2) + depth / 2 + 2.5
    return 1.01 * ulps * EPS
