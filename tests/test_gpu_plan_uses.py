"""Every kind of MFCC plan against every use of a plan (tests/plan_uses.py): return code, dsp_last_error() and the bytes of the
outputs equal what tests/golden/plan_uses.json recorded before the plans' kernel forms and acceptance rules moved into one table.

The exception is the fixture's closed list "now_einval": calls with int16 input on a 512-point plan whose shape has no int16 form,
which passed every host check and came back as DSP_EHIP "invalid configuration argument" from the launcher's fall-through.  They are
DSP_EINVAL now, with a message that names the shapes that have the form, and a stream session for such input is refused when it is
created, not at its first push.  Refused cells return from host code before a kernel is launched."""
import json

import pytest

from tests import plan_uses as P

pytestmark = pytest.mark.gpu

NO_INT16_FORM = "PCM16 ingestion on a 512-point plan: of the kernel's shapes, MFCC rows take int16 clips and ragged batches for n_mfcc <= 16"


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def fixture():
    with open(P.FIXTURE) as f:
        return json.load(f)


def test_fixture_is_the_whole_matrix(fixture):
    assert list(fixture["plans"]) == P.PLAN_NAMES
    marked = []
    for name, cells in fixture["plans"].items():
        assert list(cells) == P.USES
        marked += [f"{name}/{use}" for use, c in cells.items() if c.get("now_einval")]
        for use, c in cells.items():
            assert bool(c.get("now_einval")) == (c["rc"] == P.DSP_EHIP), (name, use)      # nothing else was a HIP error
    assert marked == fixture["now_einval"] and len(marked) == 40
    assert fixture["unstable_hashes"] == []
    # the marked cells are int16 uses of the 512-point shapes other than (4, 10, 3)
    from tests import mfcc512_shapes as M
    for m in marked:
        name, use = m.split("/")
        assert name.startswith("shape:") and M.SHAPES[name[6:]][1][:3] != (4, 10, 3) and "pcm16" in use


@pytest.mark.parametrize("name", P.PLAN_NAMES)
def test_plan_answers_every_use_as_recorded(torch_cuda, golden, fixture, name):
    want = fixture["plans"][name]
    got = P.run_plan(torch_cuda, name, dict(golden("stop_model.npz")))
    for use in P.USES:
        w, g = want[use], got[use]
        print(f"{name}/{use}: rc {g['rc']} {g['error'][:100]!r}")
        if w.get("now_einval"):
            if use == "stream_pcm16_push":      # the session is refused at its creation
                g = got["stream_pcm16_create"]
                assert got[use] == {"rc": None, "error": "not created"}, (name, use, got[use])
            assert g["rc"] == P.DSP_EINVAL and g["error"].startswith(NO_INT16_FORM), (name, use, g)
        elif use == "stream_pcm16_create" and want["stream_pcm16_push"].get("now_einval"):
            pass      # checked with its push
        else:
            assert g == w, (name, use, g, w)

