"""include/fqss.h, fqss_hd_repitch, restated in NumPy int64 for the repitch tests: one stream at a time, no device."""
import numpy as np

HS, V, R, J = 1536, 512, 512, 32


def _x(x, i):
    """x[i] with zeros outside [0, T_in); x int64 [T_in, C]"""
    out = np.zeros((len(i), x.shape[1]), np.int64)
    ok = (i >= 0) & (i < x.shape[0])
    out[ok] = x[i[ok]]
    return out


def repitch_stream(x, T_rp, P, Q, A, hq):
    """x int16 [T_in, C], hq int [Q, J] -> (y int16 [T_rp, C], positions p_m as a list): a stream that is on"""
    x, hq, ar = x.astype(np.int64), np.asarray(hq, np.int64), np.arange
    M = (((T_rp - 1) * P) // Q + J // 2) // HS + 1
    z = np.zeros((J + M * HS, x.shape[1]), np.int64)                 # z512, index 0 at row J: zeros below
    z[J:J + HS] = V * _x(x, ar(HS))
    p = [0]
    for m in range(1, M):
        n = (m * HS * A) >> 16
        t = _x(x, p[-1] + HS + ar(V))
        w = np.lib.stride_tricks.sliding_window_view(_x(x, n - R + ar(2 * R + V)), V, axis=0)      # [2R + 1, C, V]
        cost = ((w - t.T[None]) ** 2).sum(axis=(1, 2))
        p.append(n - R + int(np.argmin(cost)))                        # argmin: the first, so the lowest d among equal costs
        i = ar(V)[:, None]
        z[J + m * HS:J + m * HS + V] = (V - i) * t + i * _x(x, p[-1] + ar(V))
        z[J + m * HS + V:J + (m + 1) * HS] = V * _x(x, p[-1] + V + ar(HS - V))
    n = ar(T_rp)
    c, phi = (n * P) // Q, (n * P) % Q
    taps = z[(J + c - J // 2 + 1)[:, None] + ar(J)[None, :]]          # [T_rp, J, C]
    acc = (hq[phi][:, :, None] * taps).sum(axis=1)
    return np.clip((acc + (1 << 23)) >> 24, -32768, 32767).astype(np.int16), p


def repitch_batch(pcm, T_rp, on, pitch, A, ratios, taps):
    """pcm int16 [B, S, T_in, C] and the [B, S] rows -> (out int16 [B, S, T_rp, C], pos int32 [B, S, M]), M as the library sizes it"""
    B, S, _, C = pcm.shape
    M = (((T_rp - 1) * 55) // 49 + J // 2) // HS + 1
    out, pos = np.zeros((B, S, T_rp, C), np.int16), np.zeros((B, S, M), np.int32)
    for b in range(B):
        for s in range(S):
            if not on[b, s]:
                out[b, s] = pcm[b, s, :T_rp]
                continue
            P, Q = ratios[int(pitch[b, s])]
            out[b, s], p = repitch_stream(pcm[b, s], T_rp, P, Q, int(A[b, s]), taps(P, Q))
            pos[b, s, :len(p)] = p
    return out, pos
