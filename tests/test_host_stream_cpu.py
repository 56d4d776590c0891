"""CPU: the host pipeline's parts that need no device -- the chunk planner (dsp_host_plan_chunks = dsp_amd/csrc/host_chunks.hpp) over
seeded random batches, the checks every new entry makes before a device is touched, the exports, and host_chunks.hpp on its own in a
stand-alone program under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import dsp_amd
from dsp_amd import lib as dl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LP = dl.LP
EINVAL = -1
HOST_SYMBOLS = ["dsp_mfcc_clips_pcm16_host", "dsp_mfcc_clips_ragged_host", "dsp_mfcc_clips_ragged_pcm16_host", "dsp_host_alloc", "dsp_host_free",
                "dsp_host_pipeline_set", "dsp_host_pipeline_get", "dsp_host_pipeline_release", "dsp_host_pipeline_stats", "dsp_host_plan_chunks"]


def _check_tiling(first, n_items):
    assert first[0] == 0 and first[-1] == n_items and (np.diff(first) > 0).all()      # in order, no empty chunk, nothing left out


def test_uniform_chunks_hold_the_floor_of_chunk_over_item_and_at_least_one():
    rng = np.random.default_rng(71)
    for _ in range(200):
        n = int(rng.integers(1, 5000))
        item = int(rng.integers(1, 300_000))
        chunk = int(rng.integers(4096, 1 << 20))
        first = dsp_amd.plan_host_chunks(n, item, chunk)
        _check_tiling(first, n)
        per = max(1, chunk // item)
        counts = np.diff(first)
        assert (counts[:-1] == per).all() and 1 <= counts[-1] <= per and len(counts) == -(-n // per)
    assert dsp_amd.plan_host_chunks(37, 4000, 5 * 4000).tolist() == [0, 5, 10, 15, 20, 25, 30, 35, 37]
    assert dsp_amd.plan_host_chunks(3, 1 << 20, 4096).tolist() == [0, 1, 2, 3]                # an item larger than a chunk: one per chunk
    assert dsp_amd.plan_host_chunks(1000, 64000, 32 << 20).tolist() == [0, 524, 1000]
    assert dsp_amd.plan_host_chunks(100, 64000, 1 << 30).tolist() == [0, 100]                  # chunk_bytes above the batch: one chunk
    assert dsp_amd.plan_host_chunks(0, 64000, 4096).tolist() == [0]                            # no item, no chunk


def test_ragged_chunks_cut_at_clip_boundaries_only():
    rng = np.random.default_rng(72)
    for trial in range(200):
        n = int(rng.integers(1, 400))
        bps = int(rng.choice([2, 4, 8]))
        chunk = int(rng.integers(4096, 200_000))
        lengths = rng.integers(0, 2 * chunk // bps // 3, n)
        lengths[rng.random(n) < 0.2] = 0                                                    # empty clips, runs of them included
        if trial % 3 == 0:
            lengths[int(rng.integers(0, n))] = chunk // bps + int(rng.integers(1, 5000))    # a clip longer than a chunk
        offsets = np.concatenate([[int(rng.integers(0, 9))], lengths]).cumsum()
        first = dsp_amd.plan_host_chunks(n, bps, chunk, offsets)
        _check_tiling(first, n)                                                             # whole clips (no clip is split), empty ones kept
        size = lengths * bps
        for k in range(len(first) - 1):
            c0, c1 = int(first[k]), int(first[k + 1])
            mine = size[c0:c1]
            if mine.sum() > chunk:                                                          # only an over-long clip goes past chunk_bytes,
                assert (mine > 0).sum() == 1 and mine.max() > chunk                         # and it is the chunk's only clip with samples
            if k + 1 < len(first) - 1:                                                      # greedy: the next chunk's first clip did not fit
                nxt = size[c1]
                assert nxt > 0 and mine.sum() + nxt > chunk
                assert mine.sum() > 0 or c0 == 0                                            # an empty clip never opens a chunk of its own
    assert dsp_amd.plan_host_chunks(6, 4, 4096, [0, 0, 500, 3000, 3000, 3100, 3200]).tolist() == [0, 2, 4, 6]
    assert dsp_amd.plan_host_chunks(4, 4, 1 << 20, [5, 5, 900, 900, 4000]).tolist() == [0, 4]   # chunk_bytes above the batch: one chunk
    assert dsp_amd.plan_host_chunks(3, 2, 4096, [0, 0, 0, 0]).tolist() == [0, 3]                 # nothing but empty clips: they ride together


def test_planner_refusals_name_the_argument():
    L = dl.load()
    first = np.zeros(8, np.int64)
    fp = first.ctypes.data_as(LP)
    off = np.array([0, 10, 5], np.int64).ctypes.data_as(LP)
    for args, word in (((-1, 4, None, 4096, fp, 8), "n_items"), ((3, 0, None, 4096, fp, 8), "item_bytes"), ((3, 4, None, 4095, fp, 8), "chunk_bytes"),
                       ((3, 4, None, 4096, fp, 0), "max_first"), ((2, 4, off, 4096, fp, 8), "offsets"), ((30, 4096, None, 4096, fp, 8), "first has room for 8")):
        assert L.dsp_host_plan_chunks(*args) == EINVAL and word in dl.last_error(), args
    assert L.dsp_host_plan_chunks(30, 4096, None, 4096, None, 0) == 30                     # first NULL: the count alone


def test_new_entries_refuse_before_a_device_is_touched():
    L = dl.load()
    one = np.zeros(2, np.int64).ctypes.data_as(LP)
    assert L.dsp_mfcc_clips_pcm16_host(None, None, 1, 400, 400, 1, 0, None, 1) == EINVAL and "plan is NULL" in dl.last_error()
    assert L.dsp_mfcc_clips_ragged_host(None, None, 1, one, 1, None) == EINVAL and "plan is NULL" in dl.last_error()
    assert L.dsp_mfcc_clips_ragged_pcm16_host(None, None, 1, one, 1, 0, 1, None) == EINVAL and "plan is NULL" in dl.last_error()
    p = C.c_void_p(1)
    assert L.dsp_host_alloc(0, 64, None) == EINVAL and "out is NULL" in dl.last_error()
    assert L.dsp_host_alloc(0, 0, C.byref(p)) == EINVAL and "bytes" in dl.last_error() and p.value is None
    assert L.dsp_host_alloc(-1, 64, C.byref(p)) == EINVAL and "device" in dl.last_error()
    L.dsp_host_free(None)
    cfg = dl.HostPipelineConfig()
    for bad, word in (((4095, 2, 0, 1), "chunk_bytes"), ((1 << 20, 0, 0, 1), "depth"), ((1 << 20, 5, 0, 1), "depth"), ((1 << 20, 2, 4, 1), "pageable_mode"),
                      ((1 << 20, 2, -1, 1), "pageable_mode"), ((1 << 20, 2, 0, 0), "classify_min_clips")):
        cfg.chunk_bytes, cfg.depth, cfg.pageable_mode, cfg.classify_min_clips = bad
        assert L.dsp_host_pipeline_set(0, C.byref(cfg)) == EINVAL and word in dl.last_error(), bad
    for device in (-1, 64):
        assert L.dsp_host_pipeline_set(device, None) == EINVAL and "device" in dl.last_error()
        assert L.dsp_host_pipeline_get(device, C.byref(cfg)) == EINVAL and L.dsp_host_pipeline_release(device) == EINVAL
        assert L.dsp_host_pipeline_stats(device, C.byref(dl.HostStats())) == EINVAL
    assert L.dsp_host_pipeline_get(0, None) == EINVAL and "cfg is NULL" in dl.last_error()
    assert L.dsp_host_pipeline_stats(0, None) == EINVAL and "out is NULL" in dl.last_error()


def test_pipeline_settings_are_kept_per_device_without_a_device():
    try:
        defaults = dsp_amd.host_pipeline(5)
        assert defaults[0] >= 16 << 20 and 1 <= defaults[1] <= 4      # "tens of MB": far above any test batch
        assert defaults[2] == dl.PAGEABLE_WHOLE and defaults[3] >= 64
        assert dsp_amd.host_pipeline(5, chunk_bytes=8192) == (8192,) + defaults[1:]
        assert dsp_amd.host_pipeline(5, depth=1, pageable_mode=dl.PAGEABLE_STAGE) == (8192, 1, 0, defaults[3])
        assert dsp_amd.host_pipeline(6, depth=2, classify_min_clips=1) == (defaults[0], 2, defaults[2], 1)      # another device's pipeline, its own settings
        with pytest.raises(dsp_amd.DspError, match="depth must be 1 .. 4"):
            dsp_amd.host_pipeline(5, depth=9)
        assert dsp_amd.host_pipeline(5, depth=4, chunk_bytes=4096) == (4096, 4, 0, defaults[3])
        # the same values set one by one are the defaults: nothing depends on how a configuration was set
        assert dsp_amd.host_pipeline(5, chunk_bytes=defaults[0], depth=defaults[1], pageable_mode=defaults[2]) == defaults
        st = dsp_amd.host_pipeline_stats(5)
        assert st["n_chunks"] == 0 and st["bytes_h2d"] == 0 and st["pinned_ring_bytes"] == 0   # no host call has run there
        dsp_amd.host_pipeline_release(5)                                                    # never opened: nothing to return
    finally:
        assert dsp_amd.host_pipeline(5) == defaults and dsp_amd.host_pipeline(6) == defaults


def test_host_symbols_declared_exported_and_listed():
    with open(os.path.join(ROOT, "include", "dsp_amd.h")) as f:
        header = f.read()
    L = dl.load()
    nm = subprocess.run(["nm", "-D", "--defined-only", dl._build.LIB], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (\w+)$", nm, re.M))
    for name in HOST_SYMBOLS:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in dl.SYMBOLS and hasattr(L, name) and name in exported, name
    assert C.sizeof(dl.HostPipelineConfig) == 24 and C.sizeof(dl.HostStats) == 56
    for name in ("host_chunks.hpp", "host_pipe.hpp", "capi_host.cpp"):                      # part of the library's source hash
        assert name in dl._build.SOURCES + dl._build.HEADERS


def test_wrappers_take_numpy_arrays_and_cpu_tensors_without_a_copy():
    import torch
    a = np.arange(12, dtype=np.float32).reshape(3, 4)
    assert dl.host_array(a, np.float32) is a
    t = torch.arange(12, dtype=torch.float32).reshape(3, 4)
    assert dl.host_array(t, np.float32).ctypes.data == t.data_ptr()                         # the tensor's own memory (a pinned one stays pinned)
    assert dl.host_array(a[:, ::2], np.float32).flags.c_contiguous and dl.host_array(a.astype(np.float64), np.float32).dtype == np.float32


SANITIZED_MAIN = r"""
// host_chunks.hpp on its own: the planner's and the layouts' properties over seeded batches, for the sanitizers to watch.
// Every property has an exit code of its own.
#include <cstdio>
#include <cstdint>
#include <vector>
#include "host_chunks.hpp"

static uint64_t state = 0x9E3779B97F4A7C15ull;
static uint64_t next() { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return state; }

using namespace dsp::host;

// a planned ragged layout: every chunk starts on four samples at or just below its first clip, its rebased offsets describe exactly
// its bytes, and the chunks cover the batch with nothing but the alignment's overlap between them
static int check_ragged(const RaggedLayout &l)
{
    const long *off = l.offsets, bps = (long)l.bytes_per_sample, n_chunks = (long)l.first.size() - 1;
    std::vector<long> rebased;
    for (long k = 0; k < n_chunks; ++k) {
        const long c0 = l.first[(size_t)k], s = l.start(k), width = (long)l.chunk_width(k);
        if (s % 4 != 0) return 11;
        if (s < off[c0] - 3 || s > off[c0]) return 12;
        l.rebase(k, rebased);
        if ((long)rebased.size() != l.first[(size_t)k + 1] - c0 + 1) return 13;
        for (size_t c = 0; c + 1 < rebased.size(); ++c)
            if (rebased[c + 1] < rebased[c]) return 13;
        if (rebased[0] < 0 || rebased[0] > 3) return 14;
        if (rebased.back() * bps != width) return 15;
        if ((long)l.src_offset(k) != s * bps || l.rows(k) != 1) return 18;
        if (k + 1 < n_chunks && l.start(k + 1) * bps < s * bps + width - 3 * bps) return 17;
        if (k + 1 < n_chunks && l.start(k + 1) * bps > s * bps + width) return 17;          // (a gap: samples lost)
    }
    if ((long)l.base_offset() != l.start(0) * bps || (long)l.extent() != (off[l.n_clips] - l.start(0)) * bps) return 16;
    return 0;
}

// a planned uniform layout: the chunks' rows end where the batch ends, and staging holds them dst_pitch apart
static int check_uniform(const UniformLayout &l)
{
    const long n_chunks = (long)l.first.size() - 1;
    size_t rows = 0;
    for (long k = 0; k < n_chunks; ++k) {
        const size_t r = l.rows(k);
        if (r < 1 || l.chunk_width(k) != l.width) return 23;
        if (l.staged_bytes(k) != l.dst_pitch * (r - 1) + l.width) return 21;
        if (r == 1 && l.staged_bytes(k) != l.width) return 22;
        if (l.src_offset(k) != rows * l.src_pitch) return 23;
        rows += r;
    }
    if (rows != (size_t)l.n_items || l.base_offset() != 0) return 23;
    if (l.src_offset(n_chunks - 1) + (l.rows(n_chunks - 1) - 1) * l.src_pitch + l.width != l.extent()) return 20;
    return 0;
}

int main()
{
    std::vector<long> first;
    long chunks = 0;
    for (int trial = 0; trial < 2000; ++trial) {
        const long n = (long)(next() % 300), bps = 1L << (next() % 4), chunk = kMinChunkBytes + (long)(next() % 100000);
        std::vector<long> off((size_t)n + 1);
        off[0] = (long)(next() % 7);
        for (long c = 0; c < n; ++c) {
            long len = next() % 5 == 0 ? 0 : (long)(next() % (unsigned long)(chunk / bps));
            if (next() % 50 == 0) len += chunk;
            off[(size_t)c + 1] = off[(size_t)c] + len;
        }
        if (!plan_ragged(off.data(), n, bps, chunk, first)) return 1;
        if (first.front() != 0 || first.back() != n || (n == 0 && first.size() != 1)) return 2;
        for (size_t k = 0; k + 1 < first.size(); ++k) {
            if (first[k + 1] <= first[k]) return 3;
            long bytes = 0, with_samples = 0;
            for (long c = first[k]; c < first[k + 1]; ++c) { bytes += (off[(size_t)c + 1] - off[(size_t)c]) * bps; with_samples += off[(size_t)c + 1] > off[(size_t)c]; }
            if (bytes > chunk && with_samples != 1) return 4;
        }
        chunks += (long)first.size() - 1;
        const long item = 1 + (long)(next() % 200000), max_items = (long)(next() % 3) * 7;
        plan_uniform(n, item, chunk, first, max_items);
        if (first.front() != 0 || first.back() != n) return 5;
        for (size_t k = 0; k + 1 < first.size(); ++k)
            if (first[k + 1] <= first[k]) return 6;
        chunks += (long)first.size() - 1;
        if (n == 0) continue;                  // (a layout is a batch with at least one item: the entries return before they make one)
        // the layouts over the same batches: the same plans, and the bytes they place
        RaggedLayout rl;
        rl.offsets = off.data(); rl.n_clips = n; rl.bytes_per_sample = (size_t)bps;
        if (rl.base_offset() % (4 * (size_t)bps) != 0 || (long)rl.base_offset() > off[0] * bps) return 10;      // (asked before there is a plan)
        rl.plan(chunk);
        std::vector<long> again;
        plan_ragged(off.data(), n, bps, chunk, again);
        if (rl.first != again) return 10;
        if (const int rc = check_ragged(rl)) return rc;
        UniformLayout ul;
        ul.n_items = n; ul.dst_pitch = (size_t)item; ul.src_pitch = (size_t)item + (size_t)(next() % 64); ul.width = 1 + (size_t)(next() % (unsigned long)item);
        ul.plan(chunk, max_items);
        if (ul.first != first) return 19;
        if (const int rc = check_uniform(ul)) return rc;
    }
    {   // a single row is `width` bytes, whatever the pitches
        UniformLayout one;
        one.n_items = 1; one.src_pitch = 64000; one.dst_pitch = 64016; one.width = 63998;
        one.plan(kMinChunkBytes);
        if (one.first.size() != 2 || one.staged_bytes(0) != 63998 || one.extent() != 63998) return 22;
        if (const int rc = check_uniform(one)) return rc;
    }
    {   // far offsets and long clips: offsets[0] near 2^40, and one clip of 2^31 - 1 samples of 8 bytes (no sum may overflow)
        const long far[4] = {(1L << 40) + 3, (1L << 40) + 1003, (1L << 40) + 1003, (1L << 40) + 9002};
        RaggedLayout l;
        l.offsets = far; l.n_clips = 3; l.bytes_per_sample = 8;
        l.plan(kMinChunkBytes);
        if (l.first.size() != 3 || l.base_offset() != (size_t)8 << 40 || l.extent() != 9002 * 8) return 24;
        if (const int rc = check_ragged(l)) return rc;
        const long longest[2] = {5, 5 + (long)INT32_MAX};
        l.offsets = longest; l.n_clips = 1;
        l.plan(kMinChunkBytes);
        if (l.first.size() != 2 || l.chunk_width(0) != ((size_t)INT32_MAX + 1) * 8 || l.base_offset() != 32) return 25;
        if (const int rc = check_ragged(l)) return rc;
        UniformLayout u;                       // 2^31 clips of 64 000 bytes in one chunk
        u.n_items = 1L << 31; u.src_pitch = 64000; u.dst_pitch = 64016; u.width = 64000;
        u.plan(INT64_MAX / 4);
        if (u.first.size() != 2 || u.extent() != (((size_t)1 << 31) - 1) * 64000 + 64000) return 26;
        if (const int rc = check_uniform(u)) return rc;
    }
    // the extremes: sizes near LONG_MAX must not overflow the running sum
    const long huge[4] = {0, INT64_MAX / 8, INT64_MAX / 8 + 5, INT64_MAX / 4};
    if (!plan_ragged(huge, 3, 4, INT64_MAX / 2, first) || first.size() != 4) return 7;
    const long falling[3] = {0, 9, 4};
    if (plan_ragged(falling, 2, 4, 4096, first) || !first.empty()) return 8;
    plan_uniform(5, INT64_MAX, kMinChunkBytes, first);
    if (first.size() != 6) return 9;
    std::printf("ok %ld\n", chunks);
    return 0;
}
"""


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_planner_header_alone_under_the_sanitizers(tmp_path):
    src, exe = tmp_path / "host_chunks_main.cpp", tmp_path / "host_chunks_main"
    src.write_text(SANITIZED_MAIN)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "dsp_amd", "csrc"), str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok ") and int(r.stdout.split()[1]) > 2000 and not r.stderr, (r.returncode, r.stdout, r.stderr)
