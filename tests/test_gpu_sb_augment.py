"""`kernels.sb_augment` (fqss_sb_augment, csrc/data_ops.hip) against its statement in include/fqss.h, written in NumPy: np.roll, an fp32
left-to-right sum (the kernel's own roundings, so m is exact), the FIR in fp64, the mask, the slice.  Gates: targets and the unfiltered
mixture are bit copies (torch.equal), masked samples are exactly 0, the filtered mixture is within the running-error bound of a 101-term
fma chain on identical fp32 inputs, element by element: |got - want| <= 1.01 * 101 * 2^-24 * (|h| * |m|)[p] + 2^-149 (gamma_101; derived,
not tuned).  The cases' taps are NOT symmetric, so the checker convolves with the reversed taps: the statement is a correlation."""
import numpy as np
import pytest
import torch

from .helpers_librimix import make_librimix_tree

pytestmark = pytest.mark.gpu
TILE, C_MAX = 1024, 16
DELTA = np.eye(1, 101, 50, dtype=np.float32)[0]


def statement(srcs, shifts, h, chunks, start, T, noise=None, mix_in=None):
    """-> (m, f fp64, bound, masked, tgt) over the window; srcs: fp32 [B, L_s] arrays"""
    n = min(x.shape[1] for x in list(srcs) + [y for y in (noise, mix_in) if y is not None])
    t = [np.roll(x, k, axis=1)[:, :n] for x, k in zip(srcs, shifts)]
    m = t[0] if mix_in is None else mix_in[:, :n]
    for x in (t[1:] + ([noise[:, :n]] if noise is not None else [])) if mix_in is None else []:
        m = m + x                                                   # fp32 + fp32: one rounding, as the kernel's
    assert m.dtype == np.float32
    conv = lambda a, k: np.stack([np.convolve(r.astype(np.float64), k[::-1].astype(np.float64))[50:50 + n] for r in a])
    f, bound = conv(m, h), 1.01 * 101 * 2.0 ** -24 * conv(np.abs(m), np.abs(h)) + 2.0 ** -149
    masked = np.zeros(m.shape, dtype=bool)
    for b, lo, hi in ((b, *r) for b, row in enumerate(chunks or []) for r in row):
        masked[b, lo:hi] = True
    w = slice(start, start + T)
    return m[:, w], f[:, w], bound[:, w], masked[:, w], np.stack([x[:, w] for x in t], axis=1)


def check(srcs, shifts, h, chunks, start, T, noise=None, mix_in=None):
    from fqss_amd import kernels as K
    dev = lambda x: None if x is None else torch.from_numpy(x).cuda()
    mix, tgt = K.sb_augment([dev(x) for x in srcs], shifts, None if h is None else torch.from_numpy(h), chunks, start, T, noise=dev(noise),
                            mix_in=dev(mix_in))
    m, f, bound, masked, want_tgt = statement(srcs, shifts, DELTA if h is None else h, chunks, start, T, noise, mix_in)
    assert mix.shape == (m.shape[0], 1, T) and torch.equal(tgt.cpu(), torch.from_numpy(want_tgt))
    got = mix[:, 0].cpu().numpy()
    assert (got[masked] == 0.0).all()
    if h is None or h is DELTA:
        assert torch.equal(torch.from_numpy(got[~masked]), torch.from_numpy(m[~masked]))
    else:
        ratio = (np.abs(got.astype(np.float64) - f) / bound)[~masked].max()
        print(f"largest |got - want| / bound = {ratio:.4f}")
        assert ratio <= 1.0


def rand(seed, B, *lengths):
    g = np.random.RandomState(seed)
    return [g.uniform(-1, 1, (B, L)).astype(np.float32) for L in lengths]


TAPS = np.random.RandomState(11).uniform(-0.2, 0.2, 101).astype(np.float32)
CASES = {   # name: (B, source lengths, noise (premix: mixture) length, T_out, start (None: n - T_out), shifts, taps, premix)
    "a_left_pad": (2, (2300, 2211), None, 2 * TILE + 1, 0, (37, 2206), TAPS, False),       # last tile holds one output; wrap inside a tile
    "a_right_pad": (2, (2300, 2211), None, 2 * TILE + 1, None, (37, 2206), TAPS, False),   # start = n - T_out; source 1 wraps in a halo
    "b_scalar_store": (2, (1300, 1290, 1310), 1200, TILE - 1, 100, (5, 0, 1299), TAPS, False),
    "b_wide_store": (2, (1300, 1290, 1310), 1200, TILE, 100, (5, 0, 1299), TAPS, False),   # n = L_n
    "c_premix_filter0": (2, (1500,), 1490, 1487, 3, (0,), None, True),                       # the given mixture comes back bit for bit,
    "c_premix_delta": (2, (1500,), 1490, 1487, 3, (0,), DELTA, True),                        # through the FIR too
    "e_short": (1, (70, 64), None, 64, 0, (69, 1), TAPS, False),                             # window shorter than the halo, n = T_out
    "filter0_sum": (3, (1100, 1111), 1105, 1050, 7, (1099, 555), None, False),
}


@pytest.mark.parametrize("name", list(CASES))
def test_statement(name):
    B, Ls, Lx, T, start, shifts, h, premix = CASES[name]
    *srcs, x = rand(1, B, *Ls, Lx or 1)
    n = min(Ls + ((Lx,) if Lx else ()))
    check(srcs, shifts, h, None, n - T if start is None else start, T, **({"mix_in" if premix else "noise": x} if Lx else {}))


def test_chunks():
    """(d) chunks that start before the window, end after it, overlap, are empty, straddle a tile boundary; no chunk beside C_MAX of them"""
    start, T, srcs = 300, 2 * TILE + 40, rand(3, 2, 2600, 2590)
    rows = [(0, 310), (2300, 2590), (500, 700), (650, 900), (1000, 1000), (start + TILE - 3, start + TILE + 2), (1900, 1901)]
    rows += [(1400 + 9 * i, 1404 + 9 * i) for i in range(C_MAX - len(rows))]
    check(srcs, (0, 17), TAPS, [[], rows], start, T)
    check(srcs, (0, 17), None, [rows, []], start, T)


def test_bad_tables_raise_before_anything_is_launched():
    from fqss_amd import kernels as K
    a, b = (torch.from_numpy(x).cuda() for x in rand(4, 1, 400, 380))
    for bad in (dict(shifts=(400, 0)), dict(shifts=(-1, 0)), dict(chunks=[[(5, 381)]]), dict(chunks=[[(9, 8)]]), dict(start=81),
                dict(chunks=[[(0, 1)] * (C_MAX + 1)]), dict(taps=torch.full((101,), float("nan")))):
        with pytest.raises(ValueError, match="sb_augment"):
            K.sb_augment([a, b], **{**dict(shifts=(0, 0), taps=None, chunks=None, start=0, T_out=300), **bad})


def test_env_dataset(tmp_path):
    """both switches on: kernels.sb_augment on the tables of an identically seeded second draw; both off: the stack / sum / slice path"""
    from fqss_amd import kernels as K
    from fqss_amd.train_env.asteroid_librimix.librimix_dataset import read_wav
    from fqss_amd.train_env.speechbrain_librimix.prepare_data import SbLibriMix, draw_wavedrop, prepare_librimix
    tree = make_librimix_tree(tmp_path, n_train=3, n_dev=1, seconds=(1.2, 1.6))
    prepare_librimix(tree["data_folder"], str(tmp_path / "save"), n_spks=2)
    path, idx, cut = str(tmp_path / "save" / "libri2mix_train-360.csv"), [0, 1], 4000
    kw = dict(train=True, use_speedperturb=True, training_signal_len=cut, device="cuda")
    on = SbLibriMix(path, use_rand_shift=True, use_wavedrop=True, wavedrop={"perturb_prob": 0.0}, **kw)
    off = SbLibriMix(path, **kw)
    whole = SbLibriMix(path, device="cuda").batch(idx)[1]              # un-augmented, resampled sources: no draw
    torch.manual_seed(3)
    mix, tgt = on.batch(idx)
    assert mix.shape == (2, 1, cut) and tgt.shape == (2, 2, cut)
    torch.manual_seed(3)
    srcs = [on._perturbed(whole[:, s]) for s in range(2)]
    shifts = [int(torch.randint(-8000, 8000, (1,))) % y.shape[-1] for y in srcs]
    n = min(y.shape[-1] for y in srcs)
    lens = [len(read_wav(on.mix[i])) for i in idx]
    freqs, chunks = draw_wavedrop(on.wavedrop, n, [v / max(lens) for v in lens])
    start = int(torch.randint(0, 1 + n - cut, (1,)))
    want = K.sb_augment(srcs, shifts, torch.from_numpy(K.notch_taps(freqs)) if freqs else None, chunks, start, cut)
    assert torch.equal(mix, want[0]) and torch.equal(tgt, want[1])
    torch.manual_seed(3)
    mix, tgt = off.batch(idx)
    torch.manual_seed(3)
    outs = [off._perturbed(whole[:, s]) for s in range(2)]
    n = min(o.shape[-1] for o in outs)
    t = torch.stack([o[:, :n] for o in outs], dim=1)
    start = int(torch.randint(0, 1 + n - cut, (1,)))
    assert torch.equal(tgt, t[..., start:start + cut]) and torch.equal(mix, t.sum(1, keepdim=True)[..., start:start + cut])
