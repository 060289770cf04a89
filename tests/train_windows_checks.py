"""Shared by the training-window tests: the numpy restatement of the definitions in include/flowtimes.h ("training
windows") built on ``nbdist.philox4x32`` - keys and order, the time shift, the fp64 noise - and a builder of the
expected batch for a list of items, one item at a time.  Nothing here calls ``windows.py``."""
import numpy as np
import torch

PIECES = ("x", "y", "mask", "x_mark", "y_mark", "static", "id")
M32 = 0xFFFFFFFF


def philox_words(ftn, k, q, epoch, purpose, seed):
    """The four output words (uint64 arrays shaped like ``k`` and ``q`` broadcast) at counter
    ``(k & M32, k >> 32, q, epoch << 2 | purpose)`` and key ``(seed & M32, seed >> 32)``."""
    k = torch.from_numpy(np.asarray(k, dtype=np.int64))
    q = torch.from_numpy(np.asarray(q, dtype=np.int64))
    k, q = torch.broadcast_tensors(k, q)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    words = ftn.nbdist.philox4x32((k & M32, k >> 32, q, (int(epoch) << 2) | purpose), (seed & M32, seed >> 32))
    return [w.expand(k.shape).numpy().astype(np.uint64) for w in words]


def keys(ftn, n, seed, epoch):
    x, y, _, _ = philox_words(ftn, np.arange(n), 0, epoch, 0, seed)
    return ((x << np.uint64(32)) | y).view(np.int64)


def order(ftn, n, seed, epoch, shuffle=True):
    if not shuffle:
        return np.arange(n, dtype=np.int64)
    return np.argsort(keys(ftn, n, seed, epoch), kind="stable").astype(np.int64)


def delta(ftn, k, seed, epoch, ts):
    """The time shift of the global items ``k``: int64, in ``-ts .. ts``."""
    x = philox_words(ftn, k, 0, epoch, 1, seed)[0]
    return np.array([((int(v) * (2 * ts + 1)) >> 32) - ts for v in x.reshape(-1)], dtype=np.int64).reshape(x.shape)


def noise(ftn, k, J, seed, epoch):
    """``(z, r)`` fp64 ``[J]`` of the global item ``k``: the standard normal of element ``j`` and the Box-Muller radius
    it was made from."""
    Q = (J + 3) // 4
    a, b, c, d = philox_words(ftn, k, np.arange(Q), epoch, 2, seed)
    z = np.empty((Q, 4))
    r = np.empty((Q, 4))
    for lane, (wa, wb) in ((0, (a, b)), (2, (c, d))):
        u1 = (wa.astype(np.float64) + 0.5) * 2.0 ** -32
        u2 = (wb.astype(np.float64) + 0.5) * 2.0 ** -32
        rr = np.sqrt(-2.0 * np.log(u1))
        z[:, lane], z[:, lane + 1] = rr * np.cos(2 * np.pi * u2), rr * np.sin(2 * np.pi * u2)
        r[:, lane] = r[:, lane + 1] = rr
    return z.reshape(-1)[:J], r.reshape(-1)[:J]


def expected(ftn, parts, layout, items, seed=0, epoch=0, ts=0, sd=0.0):
    """The batch tuple (numpy arrays) of the global ``items`` over ``parts`` - dicts with X, M, marks, static, ids
    (arrays or None), L, H, stride - one item at a time; also ``radius``, the Box-Muller radius of every x element
    (zeros without noise) and ``starts``, every item's start row."""
    rows = {n: [] for n in PIECES}
    radius, starts_used = [], []
    bounds = [0]
    for p in parts:
        T, N = p["X"].shape
        W = len(range(0, T - p["L"] - p["H"] + 1, max(1, p["stride"]))) if T >= p["L"] + p["H"] else 0
        bounds.append(bounds[-1] + (W * N if layout == "series" else W))
    for k in items:
        k = int(k)
        at = next(i for i in range(len(parts)) if bounds[i] <= k < bounds[i + 1])
        p = parts[at]
        X, M, marks, L, H = p["X"], p["M"], p["marks"], p["L"], p["H"]
        T, N = X.shape
        kl = k - bounds[at]
        w, i = (kl // N, kl % N) if layout == "series" else (kl, None)
        s = w * max(1, p["stride"])
        if ts:
            s = min(max(s + int(delta(ftn, k, seed, epoch, ts)), 0), T - L - H)
        starts_used.append(s)
        e = s + L
        cut = (lambda a, lo, hi: a[lo:hi, i:i + 1]) if layout == "series" else (lambda a, lo, hi: a[lo:hi, :])
        x = cut(X, s, e)
        rad = np.zeros(x.shape)
        if sd > 0:
            z, r = noise(ftn, k, x.size, seed, epoch)
            x = (x.astype(np.float64) + np.float64(sd) * z.reshape(x.shape)).astype(np.float32)
            rad = r.reshape(x.shape)
        radius.append(rad)
        rows["x"].append(x)
        rows["y"].append(cut(X, e, e + H))
        rows["mask"].append(cut(M, e, e + H) if M is not None else np.ones_like(cut(X, e, e + H)))
        rows["x_mark"].append(marks[s:e] if marks is not None else np.zeros(0, np.float32))
        rows["y_mark"].append(marks[e:e + H] if marks is not None else np.zeros(0, np.float32))
        if layout == "series" and p["static"] is not None:
            rows["static"].append(p["static"][i:i + 1])
        if layout == "series" and p["ids"] is not None:
            rows["id"].append(p["ids"][i:i + 1])
    out = [np.stack(rows[n]) for n in PIECES if rows[n]]
    if layout == "wide":
        out += [t for t in (parts[0]["static"], parts[0]["ids"]) if t is not None]
    return out, np.stack(radius), np.array(starts_used)


def fixture_parts(arrays, meta, case):
    """The parts of a case of tests/golden/windows_cases.npz in the form ``expected`` takes."""
    out = []
    for k, p in enumerate(meta[case]["parts"]):
        t = {n: arrays.get(f"{case}:p{k}:{n}") for n in ("X", "M", "marks", "static", "ids")}
        H = p["pred_len"] if p["mode"] == "direct" else (p["recursive_pred_len"] or 1)
        t["X"] = np.asarray(t["X"], dtype=np.float32)
        out.append(dict(t, L=p["L"], H=H, stride=p["stride"]))
    return out


def spacing32(v):
    """The fp32 spacing at magnitude ``v`` (fp64 array)."""
    return np.spacing(np.abs(v).astype(np.float32)).astype(np.float64)
