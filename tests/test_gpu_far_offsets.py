"""GPU: the device entry points that take a stride, an offsets array or a row count, at positions past 2^31 elements and 2^32 bytes
(tests/far_offsets.py has the harness and the table).  Per case the far call -- the probes inside one arena of zeros, straddling and
past the boundaries -- equals the compact call on the same probes bit for bit, in every output; strided outputs land where the stride
says, between untouched sentinel bytes; and the arena is zero again once the case has zeroed what it wrote.  The arena is allocated
once per module and freed at its end.  A line of figures is printed per case (pytest -s shows them; profiles/far_offsets_gpu_tests.txt
is a copy of one run)."""
import pytest

from tests import far_offsets as FO

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def arena():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    free, need = FO.Arena.room(torch)
    if free < need:
        pytest.skip(f"the arena and its headroom need {need} bytes of free HBM, mem_get_info shows {free}")
    a = FO.Arena(torch)
    print(f"far offsets: arena of {FO.ARENA_BYTES} bytes (guard {FO.GUARD_BYTES}, payload {FO.PAYLOAD_BYTES}) zeroed in {a.alloc_ms:.1f} ms")
    yield a
    assert a.allocations == 1
    a.free()


def _by_id(id):
    return next(c for c in FO.CASES if c.id == id)


def test_the_arena_is_zero_and_scanned_quickly(arena):
    clean, ms = arena.is_zero()
    print(f"far offsets: a scan of the whole arena takes {ms:.1f} ms")
    assert clean
    assert ms < 1000.0, "the scan behind every case is too slow for a module of well under a minute"


def test_the_harness_notices_a_truncated_stride(arena, golden):
    """control: dsp_mfcc_clips_device handed stride mod 2^32 reads zeros inside the arena for the clip past 2^32"""
    import torch
    with pytest.raises(AssertionError, match="differs from the compact call"):
        FO.run_case(torch, arena, _by_id("A_mfcc_clips_512_f32"), golden, geometries=("past",), stride_error=FO.B32)
    assert arena.is_zero()[0]


def test_the_harness_notices_rows_one_stride_off(arena, golden):
    """control: a strided output whose rows the case inspects one stride behind where the call puts them fails the sentinel check"""
    import torch
    with pytest.raises(AssertionError, match="still holds the sentinel"):
        FO.run_case(torch, arena, _by_id("A_upsample_linear"), golden, geometries=("straddle",), inspect_shift=1, max_clips=2)
    assert arena.is_zero()[0]


@pytest.mark.parametrize("case", FO.CASES, ids=[c.id for c in FO.CASES])
def test_far_equals_compact(arena, golden, case):
    import torch
    for report in FO.run_case(torch, arena, case, golden):
        print(FO.line(report))          # (the far call's milliseconds are printed, not asserted: what passed FO.LIMIT_MS when measured is in NOT_REACHED)
