"""GPU: the clip augmenter (dsp_augment_*, dsp_amd.Augmenter) against the float64 restatement of its definition
(tests/augment_ref.py), stage by stage.

A float32 phase vocoder is ill-conditioned with respect to the spectrum: a bin that is nearly empty in one column takes its phase from
rounding noise and its magnitude from the neighbouring column, so float32 against float64 END TO END is mostly ~1e-6 and now and then
5e-5 (max-abs), while from THE SAME float32 spectrum the two stay within ~1e-6.  So every stage is compared with the float64 restatement
fed with the device's own bits of the stage before:

  1. STFT             device D against the restatement on the same float32 clip: per frame, max |error| over the frame's largest |D|
  2. vocoder + ISTFT  the device's D (read back from the STFT entry) through the float64 vocoder and inverse STFT, against
                      dsp_time_stretch_ragged_device: max-abs over the clip's peak
  3. ISTFT alone      a random spectrum through dsp_istft_ragged_device against the restatement
  end to end          from raw clips, by the clip's relative RMS error (max-abs is not bounded there, for the reason above)

No bound is fixed in advance: the float32 switch of the restatement runs on the same inputs, its error against the float64 restatement
is the floor, and the device is allowed 8 x that (it differs from the float32 restatement in summation order and libm only).  The floor
comes from the restatement at run time, never from the code under test.  Every (length, rate) of the grid is compared.  One addition to
that rule: a floor is never taken below 2^-24 of the metric's own normaliser, one rounding of a float32 result.  On trivial inputs (a
clip of one sample is a single impulse in its frame) the float32 restatement is EXACT, its error 0, and 8 x 0 would demand that the
device -- whose twiddles are rounded table entries, cos(pi / 2) = 6e-17 among them -- be exact too; no float32 result can be held to
less than its own rounding.

Not composed by hand: STFT -> vocoder -> ISTFT, because the vocoder has no entry of its own; the stretch entry (which is those three) is
what the apply ops are held to bit for bit, and the pitch op to stretch entry -> Resampler -> crop."""
import ctypes as C

import numpy as np
import pytest

from tests import augment_ref as A
from tests import resample_ref as R

pytestmark = pytest.mark.gpu
SR = 22050
REFLECT_LENGTHS = [1025, 1536, 2047, 2048, 2049, 2560, 5000, 22050]
ZERO_LENGTHS = [1, 511, 512, 1024]
RATES = [0.5, 0.8, 1.0, 1.2, 2.0, 196 / 185, 49 / 55]
FACTOR = 8.0
ULP = 2.0 ** -24                                                   # the least floor: one rounding of a float32 result


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return torch


def _clip(n, seed):
    """white noise at 0.3 plus a 440 Hz tone at 0.5: every bin has energy"""
    rng = np.random.default_rng(seed)
    return (0.3 * rng.standard_normal(n) + 0.5 * np.sin(2 * np.pi * 440.0 * np.arange(n) / SR)).astype(np.float32)


def _ragged(torch, clips, lead=3):
    """the clips back to back behind `lead` samples of filler (so that clips start at every alignment) -> (tensor, offsets)"""
    offs = np.concatenate([[lead], lead + np.cumsum([c.size for c in clips])]).astype(np.int64)
    return torch.from_numpy(np.concatenate([np.full(lead, 77, np.float32)] + list(clips))).cuda(), offs


def _cplx(spec_rows):
    a = spec_rows.cpu().numpy()
    return a[..., 0].astype(np.float64) + 1j * a[..., 1].astype(np.float64)


@pytest.fixture(scope="module")
def grid(torch_cuda):
    """every (pad, length, rate) once: the device's D and stretch output, and the restatement's float64 / float32 results"""
    import dsp_amd
    torch = torch_cuda
    cases = []
    for pad, lengths in (("reflect", REFLECT_LENGTHS), ("zero", ZERO_LENGTHS)):
        aug = dsp_amd.Augmenter(pad=pad)
        combos = [(n, r) for n in lengths for r in RATES]
        for b0 in range(0, len(combos), 28):                       # batches of at most 32 clips
            batch = combos[b0:b0 + 28]
            clips = [_clip(n, 100 * i + b0) for i, (n, _r) in enumerate(batch)]
            signal, offs = _ragged(torch, clips)
            spec, fo = aug.stft(signal, offs)
            out, oo = aug.time_stretch(signal, offs, [r for _n, r in batch])
            torch.cuda.synchronize()
            spec_h, out_h = _cplx(spec), out.cpu().numpy()
            for i, ((n, rate), y) in enumerate(zip(batch, clips)):
                D_dev = spec_h[fo[i]:fo[i + 1]]
                length = A.stretch_length(n, rate)
                assert oo[i + 1] - oo[i] == length and fo[i + 1] - fo[i] == A.stft_frames(n)
                D64, D32 = A.stft(y, pad), A.stft(y, pad, np.float32)
                cases.append(dict(pad=pad, n=n, rate=rate, y=y, D_dev=D_dev, out_dev=out_h[oo[i]:oo[i + 1]].astype(np.float64), D64=D64, D32=D32,
                                  from_dev64=A.istft(A.phase_vocoder(D_dev, rate), length),
                                  from_dev32=A.istft(A.phase_vocoder(D_dev.astype(np.complex64), rate, np.float32), length, np.float32),
                                  e2e64=A.istft(A.phase_vocoder(D64, rate), length),
                                  e2e32=A.istft(A.phase_vocoder(D32, rate, np.float32), length, np.float32)))
        aug.close()
    assert len(cases) == (len(REFLECT_LENGTHS) + len(ZERO_LENGTHS)) * len(RATES)
    return cases


def _frame_err(D, ref):
    return float((np.abs(D - ref).max(axis=1) / np.abs(ref).max(axis=1)).max())


def test_stft_against_float64(grid):
    worst = 0.0
    for c in grid:                                                 # (the STFT does not depend on the rate, but every clip of the grid is its own input)
        assert c["D_dev"].shape == c["D64"].shape == (A.stft_frames(c["n"]), 1025) and np.isfinite(c["D_dev"]).all()
        floor, err = max(_frame_err(c["D32"], c["D64"]), ULP), _frame_err(c["D_dev"], c["D64"])
        worst = max(worst, err / floor)
        assert err <= FACTOR * floor, (c["pad"], c["n"], c["rate"], err, floor)
    print(f"\nSTFT: worst device error / float32 floor = {worst:.3f} (allowed {FACTOR})")


def test_vocoder_and_istft_from_the_devices_spectrum(grid):
    worst, worst_abs = 0.0, 0.0
    for c in grid:
        peak = np.abs(c["from_dev64"]).max()
        floor = max(np.abs(c["from_dev32"] - c["from_dev64"]).max() / peak, ULP)
        err = np.abs(c["out_dev"] - c["from_dev64"]).max() / peak
        assert np.isfinite(c["out_dev"]).all()
        worst, worst_abs = max(worst, err / floor), max(worst_abs, err)
        assert err <= FACTOR * floor, (c["pad"], c["n"], c["rate"], err, floor)
    print(f"\nvocoder + ISTFT: worst device error / float32 floor = {worst:.3f} (allowed {FACTOR}); worst error over peak {worst_abs:.2e}")


def test_stretch_end_to_end_by_relative_rms(grid):
    worst, worst_rel = 0.0, 0.0
    for c in grid:
        norm = np.sqrt(np.mean(c["e2e64"] ** 2))
        floor = max(np.sqrt(np.mean((c["e2e32"] - c["e2e64"]) ** 2)) / norm, ULP)
        err = np.sqrt(np.mean((c["out_dev"] - c["e2e64"]) ** 2)) / norm
        worst, worst_rel = max(worst, err / floor), max(worst_rel, err)
        assert err <= FACTOR * floor, (c["pad"], c["n"], c["rate"], err, floor)
    print(f"\nend to end: worst device relative RMS / float32 floor = {worst:.3f} (allowed {FACTOR}); worst relative RMS {worst_rel:.2e}")


def test_istft_alone_on_random_spectra(torch_cuda):
    import dsp_amd
    torch = torch_cuda
    rng = np.random.default_rng(21)
    frames = [1, 3, 4, 5, 11, 44]
    lengths = [1, 1025, 1536, 2047, 512 * 11 + 700, 22050]            # (11 frames reach 6144 samples: the tail past them is the zero fill)
    specs = [(rng.standard_normal((t, 1025)) + 1j * rng.standard_normal((t, 1025))).astype(np.complex64) for t in frames]
    rows = np.concatenate(specs)
    fo = np.concatenate([[2], 2 + np.cumsum(frames)])
    buf = np.zeros((fo[-1], 1025, 2), np.float32)
    buf[2:, :, 0], buf[2:, :, 1] = rows.real, rows.imag
    buf[:2] = np.nan
    aug = dsp_amd.Augmenter(pad="zero")
    out, oo = aug.istft(torch.from_numpy(buf).cuda(), fo, lengths)
    torch.cuda.synchronize()
    got_all = out.cpu().numpy().astype(np.float64)
    worst = 0.0
    for i, S in enumerate(specs):
        got = got_all[oo[i]:oo[i + 1]]
        ref, ref32 = A.istft(S.astype(np.complex128), lengths[i]), A.istft(S, lengths[i], np.float32)
        peak = np.abs(ref).max()
        floor, err = max(np.abs(ref32 - ref).max() / peak, ULP), np.abs(got - ref).max() / peak
        assert got.shape == ref.shape
        worst = max(worst, err / floor)
        assert err <= FACTOR * floor, (frames[i], lengths[i], err, floor)
    tail = got_all[oo[4]:oo[5]][512 * 10 + 2048 - 1024:]
    assert tail.size > 0 and not tail.any()
    print(f"\nISTFT alone: worst device error / float32 floor = {worst:.3f} (allowed {FACTOR})")
    aug.close()


def test_silence_comes_out_as_exact_zeros(torch_cuda):
    import dsp_amd
    torch = torch_cuda
    aug = dsp_amd.Augmenter()
    signal = torch.zeros(3 + 3000 + 1025, device="cuda")
    out, oo = aug.time_stretch(signal, [3, 3003, 4028], [0.8, 2.0])
    assert oo.tolist() == [0, 3750, 3750 + 512] and not out.cpu().numpy().any()
    out, _ = aug.apply(signal, [3, 3003, 4028], [{"clip": 0, "kind": "pitch", "n_steps": 2}, {"clip": 1, "kind": "pitch", "n_steps": -1}])
    assert out.numel() == 4025 and not out.cpu().numpy().any()
    aug.close()


@pytest.mark.parametrize("n_steps", [1, -1, 2, -2])
def test_pitch_shift_is_the_stretch_entry_then_the_resampler(torch_cuda, n_steps):
    """output length n; the output is resample_ref on the device's own stretch output, cropped or zero filled, under the resampler
    tests' bound (L_k + 2) 2^-24 sum |h x| (tests/test_gpu_resample.py)"""
    import dsp_amd
    torch = torch_cuda
    aug = dsp_amd.Augmenter()
    up, down = dsp_amd.pitch_ratio(n_steps)
    assert (up, down) == {1: (185, 196), -1: (196, 185), 2: (49, 55), -2: (55, 49)}[n_steps]
    lens = [1025, 2049, 5000, 22050]
    clips = [_clip(n, 300 + n_steps + i) for i, n in enumerate(lens)]
    signal, offs = _ragged(torch, clips, lead=1)
    out, oo = aug.pitch_shift(signal, offs, n_steps)
    stretched, so = aug.time_stretch(signal, offs, up / down)
    torch.cuda.synchronize()
    assert np.diff(oo).tolist() == lens
    got_all, s_all = out.cpu().numpy().astype(np.float64), stretched.cpu().numpy()
    worst = 0.0
    for i, n in enumerate(lens):
        ref, mag, terms = R.resample(s_all[so[i]:so[i + 1]], down, up, with_bound=True)
        bound = A.fit((terms + 2) * 2.0 ** -24 * mag, n)
        err = np.abs(got_all[oo[i]:oo[i + 1]] - A.fit(ref, n))
        assert np.all(err <= bound), (n_steps, n, float((err / np.where(bound > 0, bound, 1)).max()))
        worst = max(worst, float((err / np.where(bound > 0, bound, np.inf)).max()))
    print(f"\npitch {n_steps:+d}: worst |err| / bound = {worst:.3f}")
    assert 0.0 < worst <= 1.0
    aug.close()


def test_a_sine_shifted_by_two_semitones(torch_cuda):
    import dsp_amd
    torch = torch_cuda
    aug = dsp_amd.Augmenter()
    y = (0.5 * np.sin(2 * np.pi * 1000.0 * np.arange(SR) / SR)).astype(np.float32)
    out, _ = aug.pitch_shift(torch.from_numpy(y).cuda(), [0, SR], 2)
    z = out.cpu().numpy().astype(np.float64)[2048:-2048]
    spec = np.abs(np.fft.rfft(z * np.hanning(z.size)))
    peak, bin_hz = np.argmax(spec) * SR / z.size, SR / z.size
    assert abs(peak - 1000.0 * 55 / 49) <= bin_hz, (peak, bin_hz)
    aug.close()


def test_noise_is_the_librarys_draws(torch_cuda):
    import dsp_amd
    torch = torch_cuda
    aug = dsp_amd.Augmenter()
    lens, sigma, seed = [1, 2, 7, 1025, 4099], 0.005, 12
    clips = [_clip(n, 500 + i) for i, n in enumerate(lens)]
    signal, offs = _ragged(torch, clips, lead=3)
    keys = [9, 2**40, 0, 5, 6]
    out, oo = aug.add_noise(signal, offs, sigma, seed=seed, keys=keys)
    again, _ = aug.add_noise(signal, offs, sigma, seed=seed, keys=keys)
    assert oo.tolist() == (offs - 3).tolist() and torch.equal(out, again)
    got_all = out.cpu().numpy().astype(np.float64)
    worst = 0.0
    for i, y in enumerate(clips):
        ref, ref32 = A.add_noise(y, np.float32(sigma), seed, keys[i]), A.add_noise(y, np.float32(sigma), seed, keys[i], np.float32)
        floor = max(np.abs(ref32 - ref).max(), ULP * np.abs(ref).max())
        err = np.abs(got_all[oo[i]:oo[i + 1]] - ref).max()
        worst = max(worst, err / floor)
        assert err <= FACTOR * floor, (lens[i], err, floor)
    print(f"\nnoise: worst device error / float32 floor = {worst:.3f} (allowed {FACTOR})")
    # 65 536 draws on silence: with a fixed seed a deterministic check, not a statistical one
    z, _ = aug.add_noise(torch.zeros(65536, device="cuda"), [0, 65536], sigma, seed=1, keys=[2])
    z = z.cpu().numpy().astype(np.float64)
    assert abs(z.mean()) <= 5 * sigma / 256 and abs(z.std() - sigma) <= 0.02 * sigma
    # sigma = 0: the source's bits, -0.0 and NaN included
    y = clips[3].copy()
    y[:3] = [-0.0, np.nan, np.float32(1e-42)]
    same, _ = aug.add_noise(torch.from_numpy(y).cuda(), [0, y.size], 0.0)
    assert np.array_equal(same.cpu().numpy().view(np.uint32), y.view(np.uint32))
    aug.close()


def test_a_clip_does_not_see_its_batch_its_order_or_the_workspace(torch_cuda):
    import dsp_amd
    torch = torch_cuda
    aug = dsp_amd.Augmenter()
    lens = [1025, 2049, 5000, 2560, 22050, 1536]
    clips = [_clip(n, 700 + i) for i, n in enumerate(lens)]
    signal, offs = _ragged(torch, clips, lead=3)
    ops = [dict(clip=0, kind="stretch", rate=0.8, key=0), dict(clip=1, kind="pitch", n_steps=2, key=1), dict(clip=2, kind="noise", sigma=0.005, key=2),
           dict(clip=2, kind="stretch", rate=1.2, sigma=0.01, key=3), dict(clip=3, kind="pitch", n_steps=-1, key=4), dict(clip=4, kind="pitch", n_steps=2, key=5),
           dict(clip=5, kind="stretch", rate=2.0, key=6), dict(clip=4, kind="pitch", n_steps=0, sigma=0.002, key=7), dict(clip=0, kind="noise", sigma=0.0, key=8)]
    out, oo = aug.apply(signal, offs, ops, seed=4)
    total = int(oo[-1])
    assert total == sum(A.out_lengths(lens, [(o["clip"], {"stretch": 0, "pitch": 1, "noise": 2}[o["kind"]], o.get("rate", 1.0), 0, 0, 0) for o in ops]))
    # a larger earlier call leaves NaN in every workspace
    big = torch.full((3 + 8 * 30000,), float("nan"), device="cuda")
    big_offs = 3 + 30000 * np.arange(9)
    junk, _ = aug.apply(big, big_offs, [dict(clip=c, kind="stretch" if c % 2 else "pitch", rate=0.5, n_steps=-2) for c in range(8)])
    assert bool(torch.isnan(junk).any())
    perm = [5, 2, 8, 0, 7, 3, 1, 6, 4]
    out_p, oo_p = aug.apply(signal, offs, [ops[j] for j in perm], seed=4)
    for pos, j in enumerate(perm):
        assert torch.equal(out_p[oo_p[pos]:oo_p[pos + 1]], out[oo[j]:oo[j + 1]]), j
    # each op alone, its clip alone at another alignment, on a fresh handle
    for j, op in enumerate(ops):
        solo = dsp_amd.Augmenter()
        one_sig, one_off = _ragged(torch, [clips[op["clip"]]], lead=j % 4)
        one, _ = solo.apply(one_sig, one_off, [dict(op, clip=0)], seed=4)
        assert torch.equal(one, out[oo[j]:oo[j + 1]]), j
        solo.close()
    # by hand: the stretch entry; the stretch entry -> Resampler -> crop or zero fill
    s0, so = aug.time_stretch(signal, offs, [0.8, 49 / 55, 1.2, 196 / 185, 49 / 55, 2.0])
    assert torch.equal(s0[so[0]:so[1]], out[oo[0]:oo[1]]) and torch.equal(s0[so[5]:so[6]], out[oo[6]:oo[7]])
    for j, c, (up, down) in ((1, 1, (49, 55)), (4, 3, (196, 185)), (5, 4, (49, 55))):
        res, ro = dsp_amd.Resampler(down, up).ragged(s0, so)
        want = torch.zeros(lens[c], device="cuda")
        piece = res[ro[c]:ro[c + 1]][:lens[c]]
        want[:piece.numel()] = piece
        assert torch.equal(want, out[oo[j]:oo[j + 1]]), j
    assert torch.equal(out[oo[8]:oo[9]], signal[offs[0]:offs[1]])
    aug.close()


def test_refusals_and_empty_calls(torch_cuda):
    import dsp_amd
    from dsp_amd import lib as dl
    torch = torch_cuda
    L = dl.load()
    aug, zero = dsp_amd.Augmenter(), dsp_amd.Augmenter(pad="zero")
    fence = torch.full((4096,), float("nan"), device="cuda")
    off = (C.c_long * 4)(0, 1024, 1024, 4000)                      # clips of 1024, 0 and 2976 samples
    huge = (C.c_long * 2)(0, 2**24)

    def op(clip, kind, rate=1.0, n_steps=0, sigma=0.0):
        return (dl.AugmentOp * 1)(dl.AugmentOp(clip, kind, rate, n_steps, sigma, 0))

    def refused(rc, word):
        assert rc == -1 and word in dl.last_error(), (rc, dl.last_error())

    p = fence.data_ptr()
    for rate in (0.1, 8.5, float("nan"), float("inf")):
        refused(L.dsp_augment_ragged_device(aug._h, p, 3, off, op(2, dl.AUGMENT_STRETCH, rate), 1, 0, p, None), "rate")
        refused(L.dsp_time_stretch_ragged_device(zero._h, p, 1, off, (C.c_double * 1)(rate), p, None), "rate")
    refused(L.dsp_augment_ragged_device(aug._h, p, 3, off, op(2, dl.AUGMENT_PITCH, n_steps=13), 1, 0, p, None), "n_steps")
    refused(L.dsp_augment_ragged_device(aug._h, p, 3, off, op(2, dl.AUGMENT_NOISE, sigma=-1.0), 1, 0, p, None), "sigma")
    refused(L.dsp_augment_ragged_device(aug._h, p, 3, off, op(3, dl.AUGMENT_NOISE), 1, 0, p, None), "clip")
    refused(L.dsp_augment_ragged_device(aug._h, p, 3, off, op(-1, dl.AUGMENT_NOISE), 1, 0, p, None), "clip")
    refused(L.dsp_augment_ragged_device(aug._h, p, 3, off, op(0, dl.AUGMENT_STRETCH), 1, 0, p, None), "1025")           # 1024 samples under reflect
    refused(L.dsp_augment_ragged_device(zero._h, p, 3, off, op(1, dl.AUGMENT_PITCH), 1, 0, p, None), "sample")          # n < 1
    refused(L.dsp_stft_ragged_device(aug._h, p, 3, off, p, None, None), "1025")
    refused(L.dsp_stft_ragged_device(zero._h, p, 3, off, p, None, None), "sample")
    refused(L.dsp_time_stretch_ragged_device(aug._h, p, 1, off, (C.c_double * 1)(1.0), p, None), "1025")
    refused(L.dsp_stft_ragged_device(zero._h, p, 1, huge, p, None, None), "2^24")
    refused(L.dsp_augment_ragged_device(zero._h, p, 1, huge, op(0, dl.AUGMENT_NOISE), 1, 0, p, None), "2^24")
    refused(L.dsp_istft_ragged_device(zero._h, p, 1, (C.c_long * 2)(0, 1), (C.c_long * 1)(2**24), p, (C.c_long * 2)(0, 0), None), "length")
    # nothing to do: DSP_OK, nothing touched
    assert L.dsp_augment_ragged_device(aug._h, p, 3, off, None, 0, 0, p, None) == 0
    assert L.dsp_augment_ragged_device(aug._h, None, 0, None, None, 0, 0, None, None) == 0
    assert L.dsp_stft_ragged_device(aug._h, None, 0, None, None, None, None) == 0
    assert L.dsp_istft_ragged_device(aug._h, None, 0, None, None, None, None, None) == 0
    assert L.dsp_time_stretch_ragged_device(aug._h, None, 0, None, None, None, None) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(fence).all())
    out, oo = aug.apply(torch.zeros(0, device="cuda"), [0], [])
    assert out.numel() == 0 and oo.tolist() == [0]
    with pytest.raises(ValueError):
        aug.time_stretch(torch.zeros(2000, device="cuda"), [0, 1000, 2000], 1.0)                                        # 1000 < 1025
    with pytest.raises(ValueError):
        aug.stft(torch.zeros(2000), [0, 2000])                                                                         # not on the GPU
    aug.close()
    zero.close()


def test_augmented_clips_train_a_scrubjay(torch_cuda):
    """16 clips plus 8 augmented ones into ScrubJay.train: a model comes back"""
    import dsp_amd
    from dsp_amd.scrubjay import ScrubJay
    torch = torch_cuda
    n = 16000
    rng = np.random.default_rng(31)
    labels = np.array([0, 1] * 8, np.int32)
    clips = [(0.1 * rng.standard_normal(n) + 0.4 * lab * np.sin(2 * np.pi * (2000.0 + 40 * i) * np.arange(n) / 16000)).astype(np.float32) for i, lab in enumerate(labels)]
    signal = torch.from_numpy(np.concatenate(clips)).cuda()
    offsets = n * np.arange(17)
    aug = dsp_amd.Augmenter()
    ops = aug.draw(labels, prob=1.0, seed=2)
    assert len(ops) == 8 and set(ops["clip"]) == set(range(1, 16, 2))
    ops["rate"] = 1.0                                              # (equal clip lengths for the 2-D batch train() takes: a stretch by 1.0 still runs the vocoder)
    extra, oo = aug.apply(signal, offsets, ops, seed=2)
    assert np.diff(oo).tolist() == [n] * 8
    x = torch.cat([signal.view(16, n), extra.view(8, n)])
    y = np.concatenate([labels, labels[ops["clip"]]])
    jay, report = ScrubJay.train(x, y)
    label, _p = jay(x)[:2]
    assert report["status"] in ("converged", "max_iter") and label.shape[0] == 24 and np.isfinite(extra.cpu().numpy()).all()
    assert set(label.cpu().numpy().tolist()) <= {0, 1}
    aug.close()
