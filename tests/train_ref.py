"""A float64 numpy restatement of ONE training step of the reference's classifier (``AMCClassifier`` in ``train()`` mode, the
loss and optimizers of ``nn_model.train_model``), and a pure-integer Philox4x32-10: what ``amcx_mlp_train_f32`` (include/amcx.h,
ABI 16.1) is held to.  tests/test_train_host.py pins it to the reference's own module in ``double()`` through the fixtures of
tests/golden/make_train_fixtures.py.

A state is a dict: ``W``, ``b`` (lists, one entry per dense layer), ``gamma``, ``beta``, ``rm``, ``rv`` (lists over the hidden
layers, None where a layer has no BatchNorm), ``slots`` (a list of one (rmsprop) or two (adam) dicts with ``W``, ``b``, ``gamma``,
``beta`` of the same shapes) and ``t``, the steps taken."""
import copy

import numpy as np

BN_EPS, BN_MOMENTUM = 1e-5, 0.1


# ---- Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11) --------------------------
def philox4x32_10(counter, key):
    """counter: four uint32 arrays (broadcastable), key: two uint32 values -> four uint32 arrays.  Integers only."""
    c = [np.asarray(v, dtype=np.uint64) for v in np.broadcast_arrays(*counter)]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    mask = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & mask, p1 >> np.uint64(32), p1 & mask
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return [v.astype(np.uint32) for v in c]


def drop_params(p):
    """(drop_threshold, keep_scale) of a dropout probability, the header's rule."""
    return int(np.rint(float(p) * 2.0 ** 32)), np.float32(1.0 / (1.0 - float(p)))


def dropout_masks(seed, t, hidden_widths, rows, threshold):
    """[bool (rows, width)] per hidden layer: unit o of row r of layer l at step count t is kept iff word o % 4 of
    Philox(counter (t mod 2^32, l, r, o // 4), key (seed low, seed high)) >= threshold."""
    out = []
    for l, width in enumerate(hidden_widths):
        r, q = np.meshgrid(np.arange(rows), np.arange((width + 3) // 4), indexing="ij")
        words = philox4x32_10((np.full_like(r, int(t) & 0xFFFFFFFF), np.full_like(r, l), r, q),
                              (int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF))
        flat = np.stack(words, axis=-1).reshape(rows, -1)[:, :width]
        out.append(flat.astype(np.uint64) >= np.uint64(threshold))
    return out


# ---- the step ---------------------------------------------------------------------------------------------------------------------
_ACT = {"relu": lambda v: np.maximum(v, 0.0), "tanh": np.tanh, "sigmoid": lambda v: 1.0 / (1.0 + np.exp(-v))}
_ACT_GRAD = {"relu": lambda y: (y > 0.0).astype(np.float64), "tanh": lambda y: 1.0 - y * y, "sigmoid": lambda y: y * (1.0 - y)}


def softmax(z):
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def new_state(W, b, gamma, beta, rm, rv, optimizer, t=0):
    f = lambda v: None if v is None else np.array(v, dtype=np.float64)
    s = {"W": [f(v) for v in W], "b": [f(v) for v in b], "gamma": [f(v) for v in gamma], "beta": [f(v) for v in beta],
         "rm": [f(v) for v in rm], "rv": [f(v) for v in rv], "t": int(t)}
    zeros = lambda vs: [None if v is None else np.zeros_like(v) for v in vs]
    s["slots"] = [{k: zeros(s[k]) for k in ("W", "b", "gamma", "beta")} for _ in range({"rmsprop": 1, "adam": 2}[optimizer])]
    return s


def _update(optimizer, lr, t, w, g, slots):
    """torch.optim.RMSprop (alpha 0.99, eps 1e-8) / torch.optim.Adam (betas 0.9 / 0.999, eps 1e-8), in place; t: this step's number."""
    if optimizer == "rmsprop":
        v = slots[0]
        v *= 0.99
        v += (1 - 0.99) * g * g
        w -= lr * g / (np.sqrt(v) + 1e-8)
    else:
        m, v = slots
        m += (g - m) * (1 - 0.9)
        v *= 0.999
        v += (1 - 0.999) * g * g
        step_size = lr / (1 - 0.9 ** t)
        w -= step_size * m / (np.sqrt(v) / np.sqrt(1 - 0.999 ** t) + 1e-8)


def step(state, x, y, *, activation, optimizer, lr, masks=None, keep_scale=1.0):
    """One step on the batch (x (rows, inputs) float64, y (rows,) int), in place.  Returns ``(summed row losses, rows whose
    argmax p is y, gradients)``, the gradients as a dict like a slot.  A row whose y lies outside the classes matches none of
    them (include/amcx.h; the reference has no such rule): no loss, never right, and dp = q / rows."""
    act, act_grad = _ACT[activation], _ACT_GRAD[activation]
    n_linear, rows = len(state["W"]), x.shape[0]
    keep_scale = float(keep_scale)
    a, inputs, cache = np.asarray(x, dtype=np.float64), [], []
    for l in range(n_linear - 1):
        inputs.append(a)
        z = a @ state["W"][l].T + state["b"][l]
        xh = rstd = None
        if state["gamma"][l] is not None:
            mu, var = z.mean(axis=0), z.var(axis=0)
            rstd = 1.0 / np.sqrt(var + BN_EPS)
            xh = (z - mu) * rstd
            state["rm"][l] = (1 - BN_MOMENTUM) * state["rm"][l] + BN_MOMENTUM * mu
            state["rv"][l] = (1 - BN_MOMENTUM) * state["rv"][l] + BN_MOMENTUM * var * rows / (rows - 1)
            z = state["gamma"][l] * xh + state["beta"][l]
        yv = act(z)
        m = np.ones_like(yv) if masks is None else masks[l].astype(np.float64)
        cache.append((xh, rstd, yv, m))
        a = yv * m * keep_scale
    inputs.append(a)
    p = softmax(a @ state["W"][-1].T + state["b"][-1])
    q = softmax(p)                                              # the reference's CrossEntropyLoss on the softmax OUTPUT
    # include/amcx.h: "a class outside 0 ... classes - 1 matches no class" -- the row's one-hot is all zero (dp = q / rows), its
    # loss term is 0 and it is never counted right.  (The header's rule alone: torch raises on such a label.)
    y = np.asarray(y, dtype=np.int64)
    inside = (y >= 0) & (y < p.shape[1])
    at = np.flatnonzero(inside)
    onehot = np.zeros_like(p)
    onehot[at, y[at]] = 1.0
    loss = float(-np.log(q[at, y[at]]).sum())
    correct = int((p.argmax(axis=1)[at] == y[at]).sum())
    dp = (q - onehot) / rows
    dz = p * (dp - (p * dp).sum(axis=1, keepdims=True))
    grads = {k: [None] * len(state[k]) for k in ("W", "b", "gamma", "beta")}
    for l in range(n_linear - 1, -1, -1):
        grads["W"][l], grads["b"][l] = dz.T @ inputs[l], dz.sum(axis=0)
        if l > 0:
            xh, rstd, yv, m = cache[l - 1]
            dv = (dz @ state["W"][l]) * m * keep_scale * act_grad(yv)
            if xh is not None:
                grads["gamma"][l - 1], grads["beta"][l - 1] = (dv * xh).sum(axis=0), dv.sum(axis=0)
                dz = state["gamma"][l - 1] * rstd * (dv - dv.mean(axis=0) - xh * (dv * xh).mean(axis=0))
            else:
                dz = dv
    state["t"] += 1
    for k in ("W", "b", "gamma", "beta"):
        for l, g in enumerate(grads[k]):
            if g is not None:
                _update(optimizer, float(lr), state["t"], state[k][l], g, [s[k][l] for s in state["slots"]])
    return loss, correct, grads


def run(state, x, y, order, batch, n_steps, **kw):
    """n_steps steps of one epoch from its start on a copy of `state`: step s takes order[s * batch : (s + 1) * batch].  ``seed``
    and ``threshold`` in place of ``masks`` draw the masks.  Returns (state, [summed losses], [right rows])."""
    state = copy.deepcopy(state)
    seed, threshold = kw.pop("seed", None), kw.pop("threshold", 0)
    losses, right = [], []
    for s in range(n_steps):
        rows = np.asarray(order[s * batch:(s + 1) * batch])
        masks = None
        if threshold:
            masks = dropout_masks(seed, state["t"], [w.shape[0] for w in state["W"][:-1]], len(rows), threshold)
        lo, ok, _ = step(state, x[rows], y[rows], masks=masks, **kw)
        losses.append(lo)
        right.append(ok)
    return state, losses, right
