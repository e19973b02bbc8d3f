"""The byte pass's 48 KiB instantiation (three 16 KiB sub-tiles per tile, the next tile's bytes
loaded in place), bit-exact against the C oracle: tokens, total and every chunk offset.

The maps are merges-file maps (every value >= 256), so they take byte mode 0, the instantiation
that runs 48 KiB tiles; every case checks through blt_debug_last_byte_tile that its launch did.

Data kinds: dense (a four-letter alphabet with all 16 pairs as merges: every wave range takes the
register path), sparse (bytes 0..7 with a random half of the pairs: the stage path) and none
(letters outside the map: a tile emits 49 152 tokens, the largest count its packed 16-bit scan
carries, and every range goes through the stage in two parts).

Sizes put the buffer end in each of the three sub-tiles and on tile edges; chunk sizes put chunk
ends in each sub-tile, on first and last positions of wave ranges and on tile edges, through both
the 32-bit chunk geometry (whole 16 KiB sub-tiles) and the 64-bit one.
"""
import numpy as np
import pytest

import blt_amd
from oracle import oracle as O

pytestmark = pytest.mark.gpu

TILE = 49152
KINDS = ("dense", "sparse", "none")
ONE_CHUNK_SIZES = (TILE - 1, TILE, TILE + 1, 32768 + 1, 32768 + 1025, TILE - 1023, 2 * TILE - 1, 5 * TILE - 3)
CHUNK_SIZES = (4096, 4097, 16384, 16385, 32768, 49152, 49153, 65543)
N_CHUNKED = 5 * TILE + 123
NMAX = 5 * TILE + 123


def _make(kind):
    rng = np.random.default_rng({"dense": 11, "sparse": 12, "none": 13}[kind])
    if kind == "dense":
        letters = [97, 98, 99, 100]
        merges = {(a, b): 256 + 4 * i + j for i, a in enumerate(letters) for j, b in enumerate(letters)}
        data = rng.integers(97, 101, NMAX, dtype=np.uint8)
    elif kind == "sparse":
        pairs = [(a, b) for a in range(8) for b in range(8)]
        keep = rng.permutation(len(pairs))[: len(pairs) // 2]
        merges = {pairs[i]: 256 + k for k, i in enumerate(sorted(keep))}
        data = rng.integers(0, 8, NMAX, dtype=np.uint8)
    else:
        letters = [97, 98, 99, 100]
        merges = {(a, b): 256 + 4 * i + j for i, a in enumerate(letters) for j, b in enumerate(letters)}
        data = rng.integers(110, 123, NMAX, dtype=np.uint8)   # no byte of the data is in a key
    return merges, data


class _Case:
    def __init__(self, kind):
        import torch
        self.merges, self.data = _make(kind)
        self.strategy = blt_amd.BpeStrategy(self.merges)
        assert (blt_amd._lib.lib().blt_debug_byte_mode(self.strategy.handle) & 0xFF) == 0
        self.oracle = O.COracle(self.merges)
        self.d_in = torch.from_numpy(self.data.copy()).cuda()
        self.d_out = torch.empty(2 * NMAX, dtype=torch.uint8, device="cuda")
        self.stream = torch.cuda.current_stream().cuda_stream

    def expect(self, n, cs):
        exp, lens = self.oracle.run(self.data[:n], cs, threads=4, return_lens=True)
        offs = np.concatenate([[0], np.cumsum(np.asarray(lens, dtype=np.int64) // 2)])
        return exp, offs

    def check(self, n, cs):
        import torch
        s = self.strategy
        nchunks = (n + cs - 1) // cs
        d_off = torch.full((nchunks + 1,), -1, dtype=torch.int64, device="cuda")
        ws_b = s.workspace_size(n, cs)
        ws = torch.full((ws_b,), 0xA5, dtype=torch.uint8, device="cuda")
        self.d_out.zero_()
        tok = s.encode_device(self.d_in.data_ptr(), n, cs, self.d_out.data_ptr(), ws.data_ptr(), ws_b, self.stream,
                              d_off.data_ptr(), sync=True)
        assert blt_amd._lib.lib().blt_debug_last_byte_tile() == TILE
        exp, offs = self.expect(n, cs)
        assert 2 * tok == exp.size
        assert np.array_equal(self.d_out[: exp.size].cpu().numpy(), exp)
        assert not self.d_out[exp.size:].any().item()   # nothing written past the tokens
        assert np.array_equal(d_off.cpu().numpy(), offs)


@pytest.fixture(scope="module", params=KINDS)
def case(request):
    return _Case(request.param)


@pytest.mark.parametrize("n", ONE_CHUNK_SIZES)
def test_one_chunk(case, n):
    case.check(n, 1 << 20)


@pytest.mark.parametrize("cs", CHUNK_SIZES)
def test_chunk_sizes(case, cs):
    case.check(N_CHUNKED, cs)


def test_back_to_back(case):
    """encode_device_prezeroed at sizes growing and shrinking on one workspace after a single
    reset: every launch exact (the self-reset zeroes the status words in 32 KiB units)."""
    import torch
    s, cs = case.strategy, 1 << 20
    sizes = (3 * TILE + 5, TILE, 1, 5 * TILE)
    ws_b = s.workspace_size(max(sizes), cs)
    ws = torch.full((ws_b,), 0xA5, dtype=torch.uint8, device="cuda")
    s.workspace_reset(ws.data_ptr(), max(sizes), cs, case.stream)
    for n in sizes:
        case.d_out.zero_()
        s.encode_device_prezeroed(case.d_in.data_ptr(), n, cs, case.d_out.data_ptr(), ws.data_ptr(), ws_b, case.stream)
        torch.cuda.synchronize()
        assert blt_amd._lib.lib().blt_debug_last_byte_tile() == TILE
        exp, _ = case.expect(n, cs)
        assert np.array_equal(case.d_out[: exp.size].cpu().numpy(), exp), n
        assert not case.d_out[exp.size:].any().item(), n
    s.check_workspace(ws.data_ptr(), case.stream)
