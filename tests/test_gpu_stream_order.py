"""GPU: every dsp_*_device entry point behind a late producer on a non-blocking side stream (tests/stream_order.py has the harness
and the table).  Per case: the outputs a consumer enqueued behind the calls copies out equal those of a quiet run on the default
stream bit for bit, the spare entries behind them are untouched, and an entry that is not documented to wait has returned while the
delay in front of its inputs was still running.  One process, two streams.  A line of figures is printed per case (pytest -s shows
them; profiles/stream_order_gpu_tests.txt is a copy of one run)."""
import pytest

from tests import stream_order as SO

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return torch


def test_the_side_stream_does_not_block(torch_cuda):
    """hipStreamGetFlags on the stream every case uses: a blocking stream would serialise with the default stream and hide everything"""
    s = SO.side_stream(torch_cuda)
    assert s.cuda_stream != torch_cuda.cuda.default_stream().cuda_stream
    assert SO.cycles_per_ms(torch_cuda) > 0


def _stats_case(run):
    """dsp_mfcc_stats_device on a small matrix, called the way `run` does it: the harness's own controls"""
    import numpy as np

    def build(golden):
        x = np.random.default_rng(5).standard_normal((5, 37, 20)).astype(np.float32)
        return None, {"x": x}
    return SO.Case("control", ("dsp_mfcc_stats_device",), build, run)


def test_the_harness_notices_work_on_another_stream(torch_cuda, golden):
    """control: the same call handed the DEFAULT stream runs at once, on the poison, and the consumer's copy differs"""
    from dsp_amd import scrubjay
    torch = torch_cuda

    def run(_, dev):
        with torch.cuda.stream(torch.cuda.default_stream()):
            return {"feat": scrubjay.mfcc_stats(dev["x"])}
    with pytest.raises(AssertionError, match="differs from the quiet run"):
        SO.run_case(torch, _stats_case(run), golden)
    torch.cuda.synchronize()


def test_the_harness_notices_a_wait(torch_cuda, golden):
    """control: a wait for the stream in front of the call, as a waiting entry would make it, and the event has completed on return"""
    from dsp_amd import scrubjay
    torch = torch_cuda

    def run(_, dev):
        torch.cuda.current_stream().synchronize()
        return {"feat": scrubjay.mfcc_stats(dev["x"])}
    with pytest.raises(AssertionError, match="waited for the stream"):
        SO.run_case(torch, _stats_case(run), golden)
    torch.cuda.synchronize()


@pytest.mark.parametrize("case", SO.CASES, ids=[c.id for c in SO.CASES])
def test_behind_a_late_producer(torch_cuda, golden, case):
    report = SO.run_case(torch_cuda, case, golden)
    text = SO.line(report)
    print(text)
    if not case.waits:
        assert report["gate_asserted_on"] == report["calls"] and len(report["returned_before_gate"]) == report["calls"]
