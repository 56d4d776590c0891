"""CPU tier: the cache policy of the frame loads, read from the gfx950 code object the build really produces.

The sources ask for non-temporal loads where frames lie back to back (every sample read once) and for plain loads where
frames overlap inside clips (csrc/stream_load.hpp).  Asking is not getting: for a long time the optimiser dropped the hint
from every instantiation of three kernels.  This test builds the library (dsp_amd.build.build() cross-compiles
without a GPU), disassembles it (tools/stream_loads.py) and looks at one thing only, the `nt` modifier on global loads and
stores.  Skipped only where the ROCm LLVM tools are missing."""
import re

import pytest

from tools import stream_loads as SL

pytestmark = pytest.mark.skipif(not SL.tools_present(), reason="llvm-objdump / llvm-objcopy of ROCm (or c++filt) not found")


@pytest.fixture(scope="module")
def kernels():
    from dsp_amd import build as B
    return SL.disassemble(B.build())


def _instances(kernels, name):
    """[(template arguments as strings, global load / store lines)] of every instantiation of dsp::<name>"""
    found = []
    for sym, lines in kernels.items():
        m = re.match(r"void dsp::" + name + r"<([^>]*)>\(", sym)
        if m:
            found.append(([a.strip() for a in m.group(1).split(",")], lines))
    assert found, f"no instantiation of {name} in the code object"
    return found


def _loads(lines, mnemonic):
    return [ins for ins in lines if ins.split()[0] == mnemonic]


def _nt(lines):
    return [ins for ins in lines if SL.is_nt(ins)]


def _check(kernels, name, clips_arg, is_frame_load_kernel=lambda args: True, mnemonic="global_load_dwordx2", at_least=1):
    """CLIPS = false: every `mnemonic` of the kernel (its only 8-byte loads are the frame's sample pairs) carries nt, and there
    are some; CLIPS = true: no load or store of the kernel carries it"""
    streaming = cached = 0
    for args, lines in _instances(kernels, name):
        if not is_frame_load_kernel(args):
            continue
        label = f"{name}<{', '.join(args)}>"
        if args[clips_arg] == "false":
            wide = _loads(lines, mnemonic)
            assert len(wide) >= at_least, f"{label}: {len(wide)} {mnemonic}, the frame loads are gone or changed width"
            plain = [ins for ins in wide if not SL.is_nt(ins)]
            assert not plain, f"{label}: {len(plain)} of {len(wide)} {mnemonic} without nt, e.g. {plain[0]}"
            streaming += 1
        else:
            assert args[clips_arg] == "true", label
            assert not _nt(lines), f"{label}: clip mode must stay cacheable, found {_nt(lines)[0]}"
            cached += 1
    assert streaming and cached, f"{name}: {streaming} streaming and {cached} clip-mode instantiations looked at"
    return streaming, cached


def test_mfcc512_wave_kernel(kernels):
    """template <DCT_SPLIT, DCT_LEN, GATHER, FLEN, IN, TILE, CLIPS, POOL, RAGGED>.  Float input: four dwordx2 per frame in flight
    and ring slot.  The launcher sends every int16 input (IN 1 .. 3) and every ragged or pooled batch through CLIPS = true, so
    no streaming instantiation reads int16; should one appear, its frame loads (dword for mono, dwordx2 for stereo) need a rule here."""
    for args, _ in _instances(kernels, "mfcc512_wave_kernel"):
        assert len(args) == 9, args
        if args[6] == "false":
            assert args[4] == "0" and args[7] == "0" and args[8] == "false", f"a streaming instantiation this test has no rule for: {args}"
    streaming, cached = _check(kernels, "mfcc512_wave_kernel", 6, at_least=4)
    assert streaming >= 28, streaming          # every (shape, FLEN, TILE) the frames entry can reach
    headline = [lines for args, lines in _instances(kernels, "mfcc512_wave_kernel") if args == ["4", "10", "3", "512", "0", "1", "false", "0", "false"]]
    assert len(headline) == 1 and len(_nt(_loads(headline[0], "global_load_dwordx2"))) == 16


def test_mfcc1024_kernel(kernels):
    """template <FULL, CLIPS>: the general 1024-point kernel, eight dwordx2 per frame"""
    _check(kernels, "mfcc1024_kernel", 1, at_least=8)


def test_mfcc2048_kernel(kernels):
    """template <CLIPS, POOL, AUB, IN, RAGGED>: float input (IN 0) is the only one that streams; the int16 front ends are clip mode"""
    for args, _ in _instances(kernels, "mfcc2048_kernel"):
        assert args[0] == "true" or args[3] == "0", args
    _check(kernels, "mfcc2048_kernel", 0, at_least=16)


def test_kernels_that_never_lost_it(kernels):
    """the same rule where the policy was a template constant from the start: mfcc1024_wave_kernel<FULL, CLIPS, PRE, ...> without the
    prefilter (PRE = true loads whole quads: dwordx4, shared with its tables) and mfcc400_kernel<CLIPS, RAGGED>"""
    _check(kernels, "mfcc1024_wave_kernel", 1, is_frame_load_kernel=lambda a: a[2] == "false", at_least=8)
    _check(kernels, "mfcc400_kernel", 0, at_least=4)
    pre = [lines for args, lines in _instances(kernels, "mfcc1024_wave_kernel") if args[1] == "false" and args[2] == "true"]
    assert pre and all(len(_nt(_loads(lines, "global_load_dwordx4"))) >= 8 for lines in pre)
