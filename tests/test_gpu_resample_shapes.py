"""GPU: every kernel form and tile geometry of the polyphase resampler by name (tests/resample_shapes.py; the classes are pinned and
the references qualified without a GPU by tests/test_resample_shapes_cpu.py).  tests/test_gpu_resample.py runs seven staged ratios to
16 kHz with 21 - 121 taps and tiles of 1024 - 4096 outputs; here run the unstaged kernel, up to 1024 branches, tiles of 4, 28 and 512
outputs, tiles that are no multiple of 16, and interleaved stereo at an odd int16 through the one-shot entries.

Per name: parity with the float64 definition through Resampler.ragged and Resampler.clips under the per-output bound of
tests/test_gpu_resample.py AND, on every recording of at least 64 outputs, the tight gate of tests/resample_shapes.py
(rms error <= MARGIN x the float32 model's rms error; MARGIN = 2); the int16 forms bit for bit against the float entry at every 16-byte
residue and at an odd int16; a recording next to NaN (full-scale) neighbours bit for bit against itself alone; impulses against the
float32 taps; and, for the staged names, live streams against the one-shot output bit for bit.

MEASURED (MI355X), rms(got - ref64) / rms(model32 - ref64), the worst recording of each name over both entries, and beside it the
worst output's share of the per-output bound.  The ratio sits at 1 (0.95 - 1.07): the kernel and the model round the same partial sums
in the same order, and the product rounding that the FMA saves is small beside them (the taps' rounding to float32, common to both, is
0.02 - 0.18 of the model's rms).  MARGIN stays 2; no kernel was found wrong.
    up1_down3 0.993 (0.23)    up1_down2 0.966 (0.20)      up1_down4 0.967 (0.11)        up1_down10 1.018 (0.16)
    up1_one_lane 1.040 (0.03) up7_one_group 0.969 (0.06)  up64_half_pass 1.073 (0.04)   cd_down 0.993 (0.22)
    cd_up 0.963 (0.29)        up3 0.959 (0.24)            up1024 1.000 (0.56)           near_unity_up 0.967 (0.40)
    near_unity_down 0.951 (0.24)  unstaged_up1 1.008 (0.06)  unstaged_up3 1.012 (0.03)  unstaged_longest 1.019 (0.27)
"""
import numpy as np
import pytest

from tests import resample_ref as R
from tests import resample_shapes as RS
from tests import stream_resample_ref as S
from tests.test_gpu_resample import _mode, _ragged, _run_ragged
from tests.test_gpu_stream_resample import _drive, _same

pytestmark = pytest.mark.gpu
INT16_FORMS = RS.FORMS[1:]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return torch


def _resampler(name):
    import dsp_amd
    rate_in, rate_out = RS.rates(name)
    rs = dsp_amd.Resampler(rate_in, rate_out)
    assert (rs.up, rs.down, rs.half) == R.ratio(rate_in, rate_out)
    return rs


def _ragged_odd(torch, sigs, lead):
    """_ragged for interleaved stereo whose first int16 lies at an odd int16 of its allocation (resample_kernel's frame-by-frame stage)"""
    filler = np.full((lead, 2), 77, np.int16)
    host = np.concatenate([filler] + list(sigs))
    offs = np.concatenate([[lead], lead + np.cumsum([s.shape[0] for s in sigs])]).astype(np.int64)
    flat = torch.zeros(1 + host.size, dtype=torch.int16, device="cuda")
    flat[1:] = torch.from_numpy(host.reshape(-1)).cuda()
    t = flat[1:].view(-1, 2)
    assert t.data_ptr() % 4 == 2 and t.is_contiguous()
    return t, offs


def _clips_odd(torch, raw):
    """one interleaved stereo clip [1][n][2] at an odd int16"""
    flat = torch.zeros(1 + raw.size, dtype=torch.int16, device="cuda")
    flat[1:] = torch.from_numpy(raw.reshape(-1).copy()).cuda()
    t = flat[1:].view(1, -1, 2)
    assert t.data_ptr() % 4 == 2
    return t


def _out_slice(rs, offs, c):
    """the output slice of recording c of a ragged batch with these input offsets"""
    oo = R.offsets(rs.rate_in, rs.rate_out, offs)
    return slice(int(oo[c]), int(oo[c + 1]))


def _split(out, oo):
    h = out.cpu().numpy()
    return [h[int(oo[c]):int(oo[c + 1])] for c in range(len(oo) - 1)]


@pytest.mark.parametrize("name", RS.NAMES)
def test_parity_under_the_bound_and_the_tight_gate(torch_cuda, name):
    torch = torch_cuda
    rs = _resampler(name)
    recs, refs = RS.recordings(name), RS.references(name)
    signal, offs = _ragged(torch, [raw for raw, _x in recs], "float")
    out, oo = _run_ragged(torch, rs, signal, offs, "float")
    worst_bound, worst_ratio, gated = 0.0, 0.0, 0
    for c, (got, (raw, _x), (ref, bound, model)) in enumerate(zip(_split(out, oo), recs, refs)):
        clip = rs.clips(torch.from_numpy(raw.copy()[None]).cuda())
        assert clip.shape == (1, ref.size) and got.shape == ref.shape
        for what, g in (("ragged", got), ("clips", clip[0].cpu().numpy())):
            err = np.abs(g.astype(np.float64) - ref)
            of_bound = float((err / np.where(bound > 0, bound, np.inf)).max()) if ref.size else 0.0
            assert np.all(np.isfinite(g)) and np.all(err <= bound), (name, raw.size, what, of_bound)
            worst_bound = max(worst_bound, of_bound)
            if model is not None:
                ratio = RS.gate_ratio(g, ref, model)
                print(f"\nresample shapes {name} n = {raw.size} ({ref.size} outputs) {what}: rms error = {ratio:.3f} x the float32 model's")
                gated += 1
                worst_ratio = max(worst_ratio, ratio)
    print(f"\nresample shapes {name}: worst rms ratio {worst_ratio:.3f} (gate {RS.MARGIN}), worst |err| / bound {worst_bound:.4f}")
    assert gated >= 2 and 0.0 < worst_bound <= 1.0
    assert worst_ratio <= RS.MARGIN, (name, worst_ratio)
    rs.close()


@pytest.mark.parametrize("name", RS.NAMES)
def test_int16_forms_are_the_float_entry_at_every_alignment(torch_cuda, name):
    """mono, stereo channel 0 and stereo average == the float entry on the decoded samples, bit for bit, with the batch starting 0 .. 7
    sample frames into its tensor (every 16-byte residue of 2-byte and 4-byte frames); stereo also from an odd int16"""
    torch = torch_cuda
    rs = _resampler(name)
    for form in INT16_FORMS:
        recs = RS.recordings(name, form)
        raws = [raw for raw, _x in recs]
        sig_f, off_f = _ragged(torch, [x for _raw, x in recs], "float", lead=0)
        want, _ = _run_ragged(torch, rs, sig_f, off_f, "float")
        for lead in range(8):
            sig_i, off_i = _ragged(torch, raws, form, lead=lead)
            got, _ = _run_ragged(torch, rs, sig_i, off_i, form)
            assert torch.equal(got, want), (name, form, lead)
        if form != "mono":
            for lead in (0, 1, 2, 3):
                sig_i, off_i = _ragged_odd(torch, raws, lead)
                got, _ = _run_ragged(torch, rs, sig_i, off_i, form)
                assert torch.equal(got, want), (name, form, "odd", lead)
            longest = max(range(len(raws)), key=lambda c: raws[c].shape[0])
            clip = rs.clips(_clips_odd(torch, raws[longest]), stereo_mode=_mode(form))
            assert torch.equal(clip[0], want[_out_slice(rs, off_f, longest)]), (name, form, "odd clip")
    rs.close()


@pytest.mark.parametrize("name", RS.NAMES)
def test_a_recording_does_not_see_poisoned_neighbours(torch_cuda, name):
    """every second recording of the batch is all NaN (float) or full scale (int16): the others are finite, and bit for bit what they
    are alone and through the clips entry"""
    torch = torch_cuda
    rs = _resampler(name)
    taps = RS.SHAPES[name][2][3]
    poison_lengths = [taps + 5, 1, 7]
    for form in RS.FORMS:
        recs = RS.recordings(name, form)
        batch = []
        for c, (raw, _x) in enumerate(recs):
            n = poison_lengths[c % 3]
            poison = np.full((n,), np.nan, np.float32) if form == "float" else np.full((n,) + raw.shape[1:], -32768, np.int16)
            batch += [poison, raw]
        batch.append(batch[0])
        signal, offs = _ragged(torch, batch, form, lead=1)
        out, oo = _run_ragged(torch, rs, signal, offs, form)
        for c, (raw, _x) in enumerate(recs):
            got = out[int(oo[2 * c + 1]):int(oo[2 * c + 2])]
            assert bool(torch.isfinite(got).all()), (name, form, raw.shape[0])
            one_sig, one_off = _ragged(torch, [raw], form, lead=c % 5)
            one, _ = _run_ragged(torch, rs, one_sig, one_off, form)
            assert torch.equal(one, got), (name, form, raw.shape[0], "alone")
            clip = rs.clips(torch.from_numpy(raw.copy()[None]).cuda(), stereo_mode=_mode(form))
            assert torch.equal(clip[0], got), (name, form, raw.shape[0], "clips")
    rs.close()


@pytest.mark.parametrize("name", RS.NAMES)
def test_impulses_give_the_float32_taps(torch_cuda, name):
    """a unit impulse at sample 0 and at n - 1: every output with one non-zero product is that float32 tap exactly -- a shifted or
    missing tap shows as itself -- and an output that both impulses reach is under the bound"""
    torch = torch_cuda
    rs = _resampler(name)
    x, want, single, ref, bound = RS.impulses(name)
    for lead in (3, 0):
        signal, offs = _ragged(torch, [x], "float", lead=lead)
        out, _ = _run_ragged(torch, rs, signal, offs, "float")
        got = out.cpu().numpy()
        assert got.shape == want.shape
        wrong = np.flatnonzero(single & (got != want))
        assert wrong.size == 0, (name, lead, wrong[:8].tolist(), got[wrong[:8]].tolist(), want[wrong[:8]].tolist())
        assert np.all(np.abs(got.astype(np.float64) - ref) <= bound), (name, lead)
    clip = rs.clips(torch.from_numpy(x.copy()[None]).cuda())
    assert np.array_equal(clip[0].cpu().numpy(), got)
    rs.close()


@pytest.mark.parametrize("fmt", ["float", "mono"])
@pytest.mark.parametrize("name", RS.STAGED_NAMES)
def test_live_streams_equal_the_one_shot_output(torch_cuda, name, fmt):
    """three streams; chunks of T - 2, T - 1 (the carry's length), T, one sample and one tile's input -+ 1, each stream in another
    order, stream 1 with nothing in every second push: pushes then finish == Resampler.ragged on the whole feed, bit for bit.  For
    up1_one_lane that is 8500 carried samples per push for 68 outputs."""
    import dsp_amd
    torch = torch_cuda
    rate_in, rate_out = RS.rates(name)
    up, down, half = R.ratio(rate_in, rate_out)
    chunks = RS.stream_chunks(name)
    assert chunks[1] == S.taps_per_branch(up, half) - 1 and min(chunks) >= 1
    cuts = [chunks[s:] + chunks[:s] for s in range(3)]
    cuts[1] = [c for pair in zip(cuts[1], [0] * len(cuts[1])) for c in pair]
    rng = RS._rng(name, 100 + len(fmt))
    feeds = [RS.signal(rng, sum(c), fmt)[0] for c in cuts]
    rs = dsp_amd.StreamResampler(rate_in, rate_out, 3, dtype=torch.float32 if fmt == "float" else torch.int16)
    got = _drive(torch, rs, feeds, cuts, fmt)
    one = _resampler(name)
    off = np.concatenate([[0], np.cumsum([len(x) for x in feeds])]).astype(np.int64)
    out, oo = one.ragged(torch.from_numpy(np.concatenate(feeds)).cuda(), off)
    want = _split(out, oo)
    n_in, n_out = rs.counts()
    for s in range(3):
        k = S.emitted(len(feeds[s]), up, down, half)
        assert n_in[s] == len(feeds[s]) and n_out[s] == k == got[s].size and k > 0
        assert _same(got[s], want[s][:k]), (name, fmt, s, k)
    rest, ro = rs.finish()
    rest = rest.cpu().numpy()
    for s in range(3):
        assert _same(np.concatenate([got[s], rest[int(ro[s]):int(ro[s + 1])]]), want[s]), (name, fmt, s)
    rs.close()
    one.close()
