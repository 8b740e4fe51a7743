"""fp64 NumPy checkers and input builders shared by tests/test_infer_batched_cpu.py and tests/test_gpu_infer_batched.py: the chunk
geometry of process.model_infer, SI-SNR with its first-maximum re-ordering scan, and the triangular overlap-add written as the plain
chunk-by-chunk loop."""
import numpy as np

# (L, seg, overlap): two overlaps, a single short chunk, no overlap, a hop that divides L - 1, an odd segment
GEOMETRIES = [(3100, 1000, 0.25), (3100, 1000, 0.75), (999, 1000, 0.25), (2000, 1000, 0.0), (1001, 500, 0.5), (1501, 333, 0.4)]
MARGIN_DB = 3.0


def geometry(L, seg, overlap):
    """(stride, N, [n_k]) of process.model_infer's chunk loop"""
    stride = int((1 - overlap) * seg)
    starts = list(range(0, L, stride))
    return stride, len(starts), [min(seg, L - s) for s in starts]


def gather_ref(mix, seg, stride, k0, G):
    L = mix.shape[-1]
    N = len(range(0, L, stride))
    out = np.zeros((G, 1, seg), np.float32)
    for g in range(G):
        k = min(k0 + g, N - 1)
        piece = mix.reshape(-1)[k * stride:k * stride + seg]
        out[g, 0, :len(piece)] = piece
    return out


def sisnr_ref(e, r):
    """torchmetrics' ScaleInvariantSignalNoiseRatio (zero-mean SI-SDR, eps = float32 eps) in fp64"""
    eps = float(np.finfo(np.float32).eps)
    e = e.astype(np.float64) - e.astype(np.float64).mean()
    r = r.astype(np.float64) - r.astype(np.float64).mean()
    alpha = (np.dot(e, r) + eps) / (np.dot(r, r) + eps)
    ts = alpha * r
    return 10.0 * np.log10((np.dot(ts, ts) + eps) / (np.dot(ts - e, ts - e) + eps))


def sisnr_chunks_ref(est, ref, seg, stride):
    """est [N, S, seg], ref [S, L] -> (db [N, S, S] fp64, map [N, S, 2], smallest best-to-second-best margin in dB)"""
    N, S, _ = est.shape
    L = ref.shape[-1]
    db = np.zeros((N, S, S))
    mp = np.zeros((N, S, 2), np.int32)
    margin = np.inf
    for k in range(N):
        n = min(seg, L - k * stride)
        for p in range(S):
            for q in range(S):
                db[k, p, q] = sisnr_ref(est[k, p, :n], ref[q, k * stride:k * stride + n])
        mp[k, :, 0], mp[k, :, 1] = np.arange(S), 1
        for p in range(S):
            best, bv = 0, -np.inf
            for q in range(S):                 # the strict `>` scan of swap_channel_order: the first maximum
                if db[k, p, q] > bv:
                    best, bv = q, db[k, p, q]
            mp[k, best] = (p, 1 if p == best else -1)
            if S > 1:
                top = np.sort(db[k, p])[::-1]
                margin = min(margin, top[0] - top[1])
    return db, mp, margin


def sisnr_case(L, seg, overlap, S, seed):
    """targets [S, L] and chunk estimates [N, S, seg] whose best target is clear in every chunk: estimate p of chunk k is a scaled,
    noisy copy of target assign[k][p]; the assignments include the identity, a swap, and two estimates claiming the same target.
    Samples past a chunk's length are NaN, so a kernel that reads them shows."""
    rs = np.random.RandomState(seed)
    stride, N, ns = geometry(L, seg, overlap)
    ref = (rs.randn(S, L) * 0.2 + 0.01).astype(np.float32)
    est = np.full((N, S, seg), np.nan, np.float32)
    for k in range(N):
        if k % 3 == 0:
            assign = list(range(S))
        elif k % 3 == 1:
            assign = list(range(S))[::-1]
        else:
            assign = [0] * S                  # every estimate claims target 0: the last one keeps it
        for p in range(S):
            t = ref[assign[p], k * stride:k * stride + ns[k]]
            est[k, p, :ns[k]] = (0.5 + 0.3 * p) * t + 0.02 * (1 + p) * rs.randn(ns[k]).astype(np.float32) - 0.03
    return ref, est


def tri_weight64(seg):
    h = seg // 2
    t = np.arange(seg)
    return np.where(t < h, t + 1, seg - t).astype(np.float64) / float(seg - h)


def ola_ref(chunks, maps, L, stride):
    """chunks [N, S, C, seg] -> [S, C, L] fp64: out[d, c, start + t] += w[t] * sign * chunk[k, src, c, t] chunk after chunk, then
    the division by the summed weights (process.py:160-183 with the re-ordering written as a gather)"""
    N, S, C, seg = chunks.shape
    w = tri_weight64(seg)
    out, ws = np.zeros((S, C, L)), np.zeros(L)
    for k in range(len(range(0, L, stride))):
        start = k * stride
        n = min(seg, L - start)
        for d in range(S):
            src, sign = (maps[k, d, 0], maps[k, d, 1]) if maps is not None else (d, 1)
            out[d, :, start:start + n] += w[:n] * (sign * chunks[k, src, :, :n].astype(np.float64))
        ws[start:start + n] += w[:n]
    return out / ws


def ola_case(L, seg, overlap, S, C, seed, pad_chunks=0):
    """random chunks [N + pad_chunks, S, C, seg] (NaN past each chunk's length and in the padding chunks) and random maps"""
    rs = np.random.RandomState(seed)
    stride, N, ns = geometry(L, seg, overlap)
    chunks = np.full((N + pad_chunks, S, C, seg), np.nan, np.float32)
    maps = np.zeros((N + pad_chunks, S, 2), np.int32)
    for k in range(N):
        chunks[k, :, :, :ns[k]] = rs.randn(S, C, ns[k]).astype(np.float32)
        maps[k, :, 0] = rs.randint(0, S, S)
        maps[k, :, 1] = rs.choice([-1, 1], S)
    return chunks, maps
