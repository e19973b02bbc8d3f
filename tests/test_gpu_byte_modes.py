"""The byte pass's 32 KiB instantiations (two 16 KiB sub-tiles per tile, the next tile's bytes in a
second register buffer): merge modes 1 and 2, with and without the live bit and the uniform
allmerge flag, and the generic byte pass (mode -1), bit-exact against the C oracle through the
device API: token count, token bytes, every chunk offset, and nothing written past the output.

Cases (test_case_maps_select_their_mode pins, without a GPU, the instantiation each map selects):
m1 (every letter pair valued below 256: single pass), m1_live ("qz" -> 'a' beside letter pairs valued
>= 256), m2 ("qz" -> 'q', a merge valued its own first byte, and a u16 key), m2_live (the same with
byte-pair keys only), allm (all 65 536 pairs) and generic (no free mark byte).

Data kinds, as in test_gpu_tile48.py: dense (four letters, all 16 pairs merge: the register path),
sparse (bytes 0..7, a random half of the pairs: the stage path) and none (bytes in no key: a tile
emits 32 768 tokens and every range goes through the stage in two parts).

Sizes put the buffer end in either sub-tile and on tile edges; chunk sizes put chunk ends on wave
range, sub-tile and tile edges through the 64-bit chunk geometry and through the 32-bit one, where
16384, 49152 and 81920 are odd numbers of sub-tiles (49152 and 81920 start chunks in the middle of
a 32 KiB tile).

The live bit: one "qz" merge alone in an input that otherwise merges nothing, at lane, wave range,
sub-tile, tile and buffer edges.  Its token merges again in the second pass, so a tile that forgets
to forward the bit leaves the output one pass short of the oracle's.

The non-GPU half also checks tests/kernel_model.py's restatement of the kernel's chunk geometry
(tile_info) against plain division at operands no GPU test can reach (32 TiB of input and more).
"""
import random

import numpy as np
import pytest

import blt_amd
from oracle import oracle as O
from tests import kernel_model as KM

gpu = pytest.mark.gpu

T = 32768
NMAX = 5 * T + 123
GUARD = 4096
ONE_CHUNK_SIZES = (T - 1, T, T + 1, 16384 + 1, 16384 + 1025, T - 1023, 2 * T - 1, 5 * T - 3)
CHUNK_SIZES = (4096, 4097, 16384, 16385, 32768, 49152, 49153, 65543, 81920)
N_CHUNKED = 5 * T + 123
LETTERS = (97, 98, 99, 100)
Q, Z = 113, 122

# case -> (extra keys of the dense and none maps, base of the pair values, mode, allmerge, live)
LETTER_CASES = {
    "m1": ({}, 200, 1, False, False),
    "m1_live": ({(Q, Z): 97}, 256, 1, False, True),
    "m2": ({(Q, Z): Q, (256, 97): 400}, 256, 2, False, False),
    "m2_live": ({(Q, Z): Q}, 256, 2, False, True),
}
KINDS = ("dense", "sparse", "none")
CASE_KINDS = [(c, k) for c in LETTER_CASES for k in KINDS] + [("allm", "allm"), ("generic", "generic")]
LONG_RUN_MAPS = {
    "m1": ({(97, 97): 200}, 1, False, False),
    "m1_live": ({(97, 97): 300, (Q, Z): 97}, 1, False, True),
    "m2_live": ({(97, 97): 300, (Q, Z): Q}, 2, False, True),
}
PROBES = {"m1_live": (Q, Z, 98), "m2_live": (Q, Z, Z)}


def _make(case, kind):
    """(merges, data, (mode, allmerge, live)) of a case and data kind."""
    rng = np.random.default_rng(1000 + CASE_KINDS.index((case, kind)))
    if case == "allm":
        merges = {(a, b): (256 * a + b + 1) & 0xFFFF for a in range(256) for b in range(256)}
        return merges, rng.integers(0, 256, NMAX, dtype=np.uint8), (1, True, True)
    if case == "generic":
        merges = {(a, 7): (a << 8) | 7 for a in range(1, 256)}
        merges[(0, 0)] = 0
        return merges, rng.choice(np.array([0, 7, 9, 200], dtype=np.uint8), NMAX), (-1, False, False)
    extra, base, mode, allm, live = LETTER_CASES[case]
    if kind == "sparse":
        pairs = [(a, b) for a in range(8) for b in range(8)]
        keep = rng.permutation(len(pairs))[: len(pairs) // 2]
        merges = {pairs[i]: base + k for k, i in enumerate(sorted(keep))}
        merges.update(extra)
        if case == "m1_live":
            merges[(Q, Z)] = 3   # a byte of the sparse keys: the value stays a key component
        data = rng.integers(0, 8, NMAX, dtype=np.uint8)
    else:
        merges = {(a, b): base + 4 * i + j for i, a in enumerate(LETTERS) for j, b in enumerate(LETTERS)}
        merges.update(extra)
        if kind == "dense":
            data = rng.integers(97, 101, NMAX, dtype=np.uint8)
        else:
            data = rng.integers(101, 113, NMAX, dtype=np.uint8)   # in no key; neither 'q' nor 'z'
    return merges, data, (mode, allm, live)


def _byte_mode(s):
    v = blt_amd._lib.lib().blt_debug_byte_mode(s.handle)
    return ((v & 0xFF) - (256 if v & 0x80 else 0), bool(v & 0x100), bool(v & 0x200))


def _u16_passes():
    return blt_amd._lib.lib().blt_debug_last_u16_passes()


class _Case:
    """One map on the device API: a strategy, its oracle, and input and output buffers of nmax bytes
    (the output with GUARD bytes behind it)."""

    def __init__(self, merges, data, mode):
        import torch
        self.merges, self.data, self.mode = merges, data, mode
        self.strategy = blt_amd.BpeStrategy(merges)
        assert _byte_mode(self.strategy) == mode
        self.single_pass = self.strategy.info()[1]
        self.oracle = O.COracle(merges)
        self.d_in = torch.from_numpy(data.copy()).cuda()
        self.d_out = torch.empty(2 * data.size + GUARD, dtype=torch.uint8, device="cuda")
        self.stream = torch.cuda.current_stream().cuda_stream

    def expect(self, data, cs):
        exp, lens = self.oracle.run(data, cs, threads=4, return_lens=True)
        offs = np.concatenate([[0], np.cumsum(np.asarray(lens, dtype=np.int64) // 2)])
        return exp, offs

    def check(self, n, cs, data=None):
        """Encodes the first n bytes (of data, if given, else of the case's own) in chunks of cs and
        checks tokens, offsets and the bytes behind the output; returns the u16 passes that ran."""
        import torch
        s = self.strategy
        d_in = self.d_in if data is None else torch.from_numpy(np.ascontiguousarray(data[:n])).cuda()
        data = self.data if data is None else data
        nchunks = (n + cs - 1) // cs
        d_off = torch.full((nchunks + 1,), -1, dtype=torch.int64, device="cuda")
        ws_b = s.workspace_size(n, cs)
        ws = torch.full((ws_b,), 0xA5, dtype=torch.uint8, device="cuda")
        self.d_out.zero_()
        tok = s.encode_device(d_in.data_ptr(), n, cs, self.d_out.data_ptr(), ws.data_ptr(), ws_b, self.stream,
                              d_off.data_ptr(), sync=True)
        L = blt_amd._lib.lib()
        assert _byte_mode(s) == self.mode
        if self.mode[0] >= 0:
            assert L.blt_debug_last_byte_tile() == T
        if not self.single_pass:
            assert L.blt_debug_last_fused() == 0   # pass 1 ran on the byte pass, not fused with pass 2
        exp, offs = self.expect(data[:n], cs)
        assert 2 * tok == exp.size
        assert np.array_equal(self.d_out[: exp.size].cpu().numpy(), exp)
        # a single pass writes its tokens only; a general map runs its later passes in place, so
        # pass-1 tokens stay behind the final ones: nothing behind the 2 n bytes of the output
        assert not self.d_out[(exp.size if self.single_pass else 2 * n):].any().item()
        assert np.array_equal(d_off.cpu().numpy(), offs)
        return 0 if self.single_pass else _u16_passes()   # (a single pass leaves the count of an earlier encode)


# ---- without a GPU -------------------------------------------------------------------------------
def test_case_maps_select_their_mode():
    """Every map of this file selects the byte-pass instantiation its case is named for (mode,
    allmerge, live), and only m1's maps are single-pass."""
    for case, kind in CASE_KINDS:
        merges, _, mode = _make(case, kind)
        s = blt_amd.BpeStrategy(merges)
        assert _byte_mode(s) == mode, (case, kind)
        assert s.info()[1] == (case == "m1"), (case, kind)
    for name, (merges, mode, allm, live) in LONG_RUN_MAPS.items():
        s = blt_amd.BpeStrategy(merges)
        assert _byte_mode(s) == (mode, allm, live), name
        assert s.info()[1] == (name == "m1"), name


def _ref_subs(S, ns, d):
    q, r = divmod(S, d)
    left = d - r if r else 0
    return (2 * ns * KM.SUB_BYTES if left > 2 * ns else left * KM.SUB_BYTES), q + (1 if r else 0)


def _ref_bytes(Tn, ns, cs):
    q, r = divmod(Tn * ns * KM.SUB_BYTES, cs)
    return min(cs - r if r else 0, 2 * ns * KM.SUB_BYTES), q + (1 if r else 0)


@pytest.mark.parametrize("ns", [2, 3])
def test_chunk_geometry_32bit_far_operands(ns):
    """tile_info's 32-bit branch (a high multiply by floor((2^32 - 1) / d) and at most two
    corrections) equals plain division for first sub-tile indices up to the largest the host admits
    to it plus a tile, at divisors up to 2^31 - 1."""
    last_sub = KM.max_first_subtile(ns)
    assert KM.SUBS_CAP - 1 - ns < last_sub <= KM.SUBS_CAP - 1 and last_sub % ns == 0
    top = last_sub + ns
    rng = random.Random(20 + ns)
    fixed = [1, 2, 3, 1023, 1024, 1025, 65535, 65536, 65537, 1 << 30, (1 << 30) + 1, (1 << 31) - 1]
    points = []
    for d in fixed:
        pts = {0, 1, d - 1, d, d + 1, 2 * d - 1, 2 * d, top, top - 1, top - 2, top - 3}
        for q in (top // d, top // d - 1):
            pts |= {q * d - 1, q * d, q * d + 1}
        points += [(S, d) for S in sorted(pts) if 0 <= S <= top]
    for _ in range(4000):
        d = rng.randrange(1, 1 << rng.randrange(1, 32))
        S = rng.choice((rng.randrange(top + 1), top - rng.randrange(min(top, 4 * d) + 1)))
        points.append((S, d))
    most = 0
    for S, d in points:
        magic = KM.M32 // d if d > 1 else 0
        bge, k0, fixes = KM.tile_info_subs(S, ns, d, magic)
        assert (bge, k0) == _ref_subs(S, ns, d), (S, d)
        most = max(most, fixes)
    assert most <= 2
    # the host's parameters: whole sub-tiles below the cap take this branch, all else the 64-bit one
    n_cap = (KM.SUBS_CAP - 1) * KM.SUB_BYTES + KM.SUB_BYTES - 1
    assert KM.byte_pass_geometry(n_cap, 3 * KM.SUB_BYTES)[:2] == (3, KM.M32 // 3)
    assert KM.byte_pass_geometry(n_cap, KM.SUB_BYTES)[:2] == (1, 0)
    assert KM.byte_pass_geometry(n_cap + 1, 3 * KM.SUB_BYTES)[:2] == (0, 0)
    assert KM.byte_pass_geometry(1 << 20, 3 * KM.SUB_BYTES + 1)[:2] == (0, 0)
    last = (top - ns) // ns
    assert KM.tile_info(last, ns, n_cap, 5 * KM.SUB_BYTES)[:2] == _ref_bytes(last, ns, 5 * KM.SUB_BYTES)


@pytest.mark.parametrize("ns", [2, 3])
def test_chunk_geometry_64bit_far_operands(ns):
    """tile_info's 64-bit branch (a high multiply by floor((2^64 - 1) / cs)) equals plain division
    for chunk sizes from 4096 to 2^40 + 1 and tiles up to 2^32 - 1."""
    rng = random.Random(30 + ns)
    tile = ns * KM.SUB_BYTES
    tmax = (1 << 32) - 1
    sizes = [4096, 4097, 6001, 16384, 16385, 49152, 49153, 65543, (1 << 20) + 1, (1 << 24), (1 << 32) - 1, 1 << 32,
             (1 << 32) + 1, (1 << 40) - 1, 1 << 40, (1 << 40) + 1]
    sizes += [rng.randrange(4096, 1 << rng.randrange(13, 41)) for _ in range(300)] + [(1 << 40) + 1 - rng.randrange(4096)
                                                                                    for _ in range(20)]
    most = 0
    for cs in sizes:
        assert 4096 <= cs <= (1 << 40) + 1
        magic = KM.byte_pass_geometry(tmax * tile, cs)[2]
        tiles = {0, 1, 2, tmax, tmax - 1, tmax - 2}
        qtop = tmax * tile // cs
        for q in (1, 2, qtop // 2, qtop - 1, qtop):
            t = q * cs // tile   # the tile that holds chunk start q, and its neighbours
            tiles |= {t - 1, t, t + 1}
        tiles |= {rng.randrange(tmax + 1) for _ in range(8)}
        for Tn in tiles:
            if 0 <= Tn <= tmax:
                bge, k0, fixes = KM.tile_info_bytes(Tn, ns, cs, magic)
                assert (bge, k0) == _ref_bytes(Tn, ns, cs), (Tn, cs)
                most = max(most, fixes)
    assert most <= 2


# ---- on the GPU ----------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=CASE_KINDS, ids=lambda ck: ck[0] if ck[0] == ck[1] else f"{ck[0]}-{ck[1]}")
def case(request):
    return _Case(*_make(*request.param))


@pytest.fixture(scope="module", params=KINDS)
def m1_case(request):
    return _Case(*_make("m1", request.param))


@pytest.fixture(scope="module", params=sorted(PROBES))
def live_case(request):
    c = _Case(*_make(request.param, "none"))
    c.probe = PROBES[request.param]
    return c


@pytest.fixture(scope="module", params=sorted(LONG_RUN_MAPS))
def run_case(request):
    merges, mode, allm, live = LONG_RUN_MAPS[request.param]
    data = np.concatenate([np.full(17, 120, np.uint8), np.full(70 * T + 3, 97, np.uint8)])
    return _Case(merges, data, (mode, allm, live))


@gpu
@pytest.mark.parametrize("n", ONE_CHUNK_SIZES)
def test_one_chunk(case, n):
    case.check(n, 1 << 20)


@gpu
@pytest.mark.parametrize("cs", CHUNK_SIZES)
def test_chunk_sizes(case, cs):
    case.check(N_CHUNKED, cs)


@gpu
@pytest.mark.parametrize("lead", [0, 1, 2, 3, 17])
@pytest.mark.parametrize("n", [T + 5, 3 * T, 70 * T + 3])
def test_long_merge_runs_cross_tiles(run_case, lead, n):
    """A run of one byte that merges with itself, pair after pair across tiles, behind 0..17 bytes
    that shift its parity (the mode-1 and mode-2 twin of test_gpu_parity's test)."""
    data = run_case.data[17 - lead: 17 + n]   # "x" * lead + "a" * n
    assert run_case.check(lead + n, 1 << 20, data=data) == 0   # (no "qz": the byte pass is final)


@gpu
def test_back_to_back(m1_case):
    """encode_device_prezeroed at sizes growing and shrinking on one workspace after a single
    reset: every launch exact (the single-pass mode-1 kernel leaves its status words zeroed)."""
    import torch
    case = m1_case
    s, cs = case.strategy, 1 << 20
    sizes = (3 * T + 5, T, 1, 5 * T)
    ws_b = s.workspace_size(max(sizes), cs)
    ws = torch.full((ws_b,), 0xA5, dtype=torch.uint8, device="cuda")
    s.workspace_reset(ws.data_ptr(), max(sizes), cs, case.stream)
    for n in sizes:
        case.d_out.zero_()
        s.encode_device_prezeroed(case.d_in.data_ptr(), n, cs, case.d_out.data_ptr(), ws.data_ptr(), ws_b, case.stream)
        torch.cuda.synchronize()
        assert blt_amd._lib.lib().blt_debug_last_byte_tile() == T
        exp, _ = case.expect(case.data[:n], cs)
        assert np.array_equal(case.d_out[: exp.size].cpu().numpy(), exp), n
        assert not case.d_out[exp.size:].any().item(), n
    s.check_workspace(ws.data_ptr(), case.stream)


def _with(data, at, bytes_):
    d = data.copy()
    k = min(len(bytes_), d.size - at)
    d[at: at + k] = bytes_[:k]
    return d


@gpu
def test_live_bit_background(live_case):
    """Nothing merges: the byte pass is final and no u16 pass runs."""
    assert live_case.check(NMAX, 1 << 20) == 0


@gpu
@pytest.mark.parametrize("p", [0, 14, 15, 1022, 1023, 16383, T - 2, T - 1, 2 * T + 7000, NMAX - 3, NMAX - 2, NMAX - 1])
def test_live_bit_one_merge(live_case, p):
    """One "qz" merge alone, at a lane edge, a wave range edge, a sub-tile edge, a tile edge, in a
    middle tile and at the buffer end (at n - 2 only "qz" fits, at n - 1 only "q"): its tile's live
    bit reaches the last tile, so the u16 passes run and merge its token with the byte behind it."""
    n = NMAX
    passes = live_case.check(n, 1 << 20, data=_with(live_case.data, p, live_case.probe))
    if p <= n - 3:
        assert passes >= 1
    if p == n - 1:
        assert passes == 0


@gpu
@pytest.mark.parametrize("cs", [4096, 4097, 16384, 49152])
def test_live_bit_chunk_cut(live_case, cs):
    """"q" on a chunk's last byte and "z" on the next chunk's first: the pair is cut, no merge is
    live and no u16 pass runs.  The whole probe just inside the chunk start: the passes run."""
    n = NMAX
    nchunks = (n + cs - 1) // cs
    for k in sorted({1, nchunks // 2}):
        b = k * cs
        assert 0 < b and b + 3 <= n
        assert live_case.check(n, cs, data=_with(live_case.data, b - 1, (Q, Z))) == 0, k
        assert live_case.check(n, cs, data=_with(live_case.data, b, live_case.probe)) >= 1, k
