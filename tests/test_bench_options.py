"""bench.py's command line: a plain run does the timed steps only (--full is off by default), and
--dump-outputs writes the output stream's tokens and chunk offsets as float .npy files (host
tensors stand in for the device buffers here; the function only indexes them)."""
import sys

import numpy as np
import pytest

import bench


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_is_not_full(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, "", 7, 2)
    a = _parse(monkeypatch, "--full", "--only-configs", "cfg2", "--dump-outputs", "d")
    assert a.full and a.only_configs == "cfg2" and a.dump_outputs == "d"


def test_only_configs_needs_full(monkeypatch):
    with pytest.raises(SystemExit):
        _parse(monkeypatch, "--only-configs", "cfg2")


def _buffers(tokens, offsets):
    import torch
    be = np.empty(2 * tokens.size + 6, np.uint8)   # room past the stream, as the caller's 2N buffer
    be[0:2 * tokens.size:2] = tokens >> 8
    be[1:2 * tokens.size:2] = tokens & 0xFF
    be[2 * tokens.size:] = 0xEE
    return torch.from_numpy(be), torch.tensor(offsets, dtype=torch.int64)


def test_dump_outputs_whole_stream(tmp_path):
    tokens = np.array([0, 1, 255, 256, 257, 0xFFFE, 0xFFFF, 97, 40000], np.int64)
    d_out, d_off = _buffers(tokens, [0, 4, 4, 9])
    bench.dump_outputs(str(tmp_path / "o"), d_out, d_off)
    tok = np.load(tmp_path / "o" / "tokens.npy")
    off = np.load(tmp_path / "o" / "chunk_offsets.npy")
    idx = np.load(tmp_path / "o" / "token_index.npy")
    assert tok.dtype == np.float32 and off.dtype == np.float64 and idx.dtype == np.float64
    assert np.array_equal(tok, tokens) and np.array_equal(off, [0, 4, 4, 9]) and np.array_equal(idx, np.arange(9))


def test_dump_outputs_sampled_and_repeatable(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_TOKENS", 64)
    tokens = (np.arange(1000, dtype=np.int64) * 7919) & 0xFFFF
    d_out, d_off = _buffers(tokens, [0, 500, 1000])
    bench.dump_outputs(str(tmp_path / "a"), d_out, d_off)
    bench.dump_outputs(str(tmp_path / "b"), d_out, d_off, rank=1, world=2)
    idx = np.load(tmp_path / "a" / "token_index.npy").astype(np.int64)
    assert idx.size == 64 and np.all(np.diff(idx) >= 0) and idx[0] >= 0 and idx[-1] < 1000
    assert np.array_equal(np.load(tmp_path / "a" / "tokens.npy"), tokens[idx])
    for name in ("tokens", "token_index", "chunk_offsets"):
        assert np.array_equal(np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.rank1.npy"))
