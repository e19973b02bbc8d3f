"""Lane-exact CPU model of merge_pass_kernel (blt_amd/csrc/bpe_kernels.hip), for tests only.

It reproduces the kernel's decomposition — 16-position lane segments, wave ballots and
prefix scans, per-(sub-tile, wave) group functions, the tile function, and the look-back
composition (done serially here) — so the algebra of the parallel scan can be checked against
the sequential oracle on CPU, without a GPU.

Below it, the byte pass's chunk geometry (tile_info) restated with the kernel's 32- and 64-bit
wrap-around arithmetic, for operands far past any input a GPU test can hold
(tests/test_gpu_byte_modes.py).
"""
from typing import Dict, Tuple

THREADS, SEG, SUB = 512, 16, 4
WAVES = THREADS // 64
SUBPOS = THREADS * SEG
TILEPOS = SUB * SUBPOS


def merges_for(m, c):
    mc = m if c else (m & ~1)
    s = mc & ~(mc << 1)
    rodd = mc & ~(mc + (s & 0xAAAA))
    return (mc & ~rodd & 0x5555) | (rodd & 0xAAAA)


def lands_for(M, c, valid):
    return ~((M << 1) | (c ^ 1)) & valid & 0xFFFF


def resolve(items):
    """items: per-lane (ident, cout, cnt0, cnt1) for 64 lanes -> per-lane (has_below, below_cout,
    excl0, excl1) and the wave function (ident, cout, cnt0, cnt1)."""
    out = []
    last_nonid_cout = None
    acc0 = acc1 = 0
    for ident, cout, c0, c1 in items:
        hb = last_nonid_cout is not None
        bc = last_nonid_cout if hb else 0
        cin0 = bc if hb else 0
        cin1 = bc if hb else 1
        out.append((hb, bc, acc0, acc1))
        acc0 += c1 if cin0 else c0
        acc1 += c1 if cin1 else c0
        if not ident:
            last_nonid_cout = cout
    fn = (last_nonid_cout is None, last_nonid_cout or 0, acc0, acc1)
    return out, fn


def run_pass(seq, merges: Dict[Tuple[int, int], int], chunk_size: int):
    """One kernel pass over positions `seq` (ints) -> output tokens."""
    n = len(seq)
    out = [None] * n
    C, O = 1, 0
    ntiles = (n + TILEPOS - 1) // TILEPOS
    for T in range(ntiles):
        tile0 = T * TILEPOS
        lanes = {}
        wfn = {}
        for j in range(SUB):
            sub0 = tile0 + j * SUBPOS
            for w in range(WAVES):
                items = []
                for l in range(64):
                    pos = sub0 + (w * 64 + l) * SEG
                    vmask = 0 if pos >= n else (0xFFFF if n - pos >= 16 else (1 << (n - pos)) - 1)
                    m = 0
                    vals = [0] * 16
                    for k in range(16):
                        p = pos + k
                        if p + 1 < n:
                            v = merges.get((seq[p], seq[p + 1]))
                            if v is not None:
                                m |= 1 << k
                                vals[k] = v
                    # the kernel's boundary walk: chunk starts b in (sub0, sub0 + SUBPOS] clear m at b - 1
                    x = sub0 + 1 if sub0 + 1 < n else n
                    kk = (x + chunk_size - 1) // chunk_size
                    b = min(kk * chunk_size, n)
                    while b < n and b <= sub0 + SUBPOS:
                        e = b - 1
                        if pos <= e < pos + 16:
                            m &= ~(1 << (e - pos))
                        b = min((kk + 1) * chunk_size, n)
                        kk += 1
                    ident = m == 0xFFFF
                    M1, M0 = merges_for(m, 1), merges_for(m, 0)
                    cnt1 = bin(lands_for(M1, 1, vmask)).count("1")
                    cnt0 = bin(lands_for(M0, 0, vmask)).count("1")
                    cout = ((M1 >> 15) & 1) ^ 1
                    items.append((ident, cout, cnt0, cnt1))
                    lanes[(j, w, l)] = (pos, m, vmask, vals)
                res, fn = resolve(items)
                for l in range(64):
                    lanes[(j, w, l)] = lanes[(j, w, l)] + res[l]
                wfn[(j, w)] = fn
        groups = [wfn[(j, w)] for j in range(SUB) for w in range(WAVES)]
        gres, tf = resolve(groups + [(True, 0, 0, 0)] * (64 - len(groups)))
        # look-back (serial): the carry/offset entering this tile are C, O
        tile_cnt = tf[3] if C else tf[2]
        for j in range(SUB):
            for w in range(WAVES):
                g = j * WAVES + w
                ghb, gbc, gx0, gx1 = gres[g]
                cg = gbc if ghb else C
                og = gx1 if C else gx0
                for l in range(64):
                    pos, m, vmask, vals, hb, bc, e0, e1 = lanes[(j, w, l)]
                    c = bc if hb else cg
                    lane_off = og + (e1 if cg else e0)
                    M = merges_for(m, c)
                    L = lands_for(M, c, vmask)
                    r = O + lane_off
                    for k in range(16):
                        if (L >> k) & 1:
                            out[r] = vals[k] if (M >> k) & 1 else seq[pos + k]
                            r += 1
        co = (1 if C else 0) if tf[0] else tf[1]
        O += tile_cnt
        C = co
    return out[:O]


# ---- the byte pass's chunk geometry (tile_info, bpe_kernels.hip) ---------------------------------
# Both branches restated with the kernel's word sizes: the 32-bit one in sub-tile units (chunk sizes
# that are whole 16 KiB sub-tiles) and the 64-bit one in bytes, each a high multiply with the host's
# reciprocal and at most two corrections.  Each returns (bge, k0, corrections): the first chunk start
# at or after the tile start, relative to it and clamped to two tiles; its chunk index; and how many
# of the two corrections ran.
SUB_BYTES = 16384          # kSubPosBytes
M32, M64 = (1 << 32) - 1, (1 << 64) - 1
SUBS_CAP = (1 << 31) - 8   # run_byte_pass: the 32-bit branch only while n / SUB_BYTES is below this


def byte_pass_geometry(n, cs):
    """(cs_subs, cs_subs_magic, cs_magic) as run_byte_pass (blt_host.cpp) fills them in."""
    cs_magic = M64 // cs
    cs_subs = cs_subs_magic = 0
    if cs % SUB_BYTES == 0 and n // SUB_BYTES < SUBS_CAP:
        cs_subs = min(cs // SUB_BYTES, 0x7FFFFFFF)
        cs_subs_magic = M32 // cs_subs if cs_subs > 1 else 0
    return cs_subs, cs_subs_magic, cs_magic


def max_first_subtile(ns):
    """The largest first sub-tile index NS T of a tile the 32-bit branch meets: the last tile of the
    longest buffer run_byte_pass admits to it (n / SUB_BYTES = SUBS_CAP - 1)."""
    n = (SUBS_CAP - 1) * SUB_BYTES + SUB_BYTES - 1
    ntiles = (n + ns * SUB_BYTES - 1) // (ns * SUB_BYTES)
    return ns * (ntiles - 1)


def tile_info_subs(S, ns, cs_subs, cs_subs_magic):
    """The 32-bit branch for a tile whose first sub-tile is S (the kernel: S = NS T), uint32 wrap-around."""
    d = cs_subs
    S &= M32
    q = S if d == 1 else (S * cs_subs_magic) >> 32   # __umulhi
    r = (S - q * d) & M32
    fixes = 0
    for _ in range(2):
        if r >= d:
            q = (q + 1) & M32
            r = (r - d) & M32
            fixes += 1
    left_subs = (d - r) & M32 if r else 0
    far = 2 * ns * SUB_BYTES
    bge = far if left_subs > 2 * ns else (left_subs * SUB_BYTES) & M32
    return bge, q + (1 if r else 0), fixes


def tile_info_bytes(T, ns, cs, cs_magic):
    """The 64-bit branch for tile T, uint64 wrap-around."""
    tile0 = (T * ns * SUB_BYTES) & M64
    q = (tile0 * cs_magic) >> 64   # __umul64hi
    r = (tile0 - q * cs) & M64
    fixes = 0
    for _ in range(2):
        if r >= cs:
            q = (q + 1) & M64
            r = (r - cs) & M64
            fixes += 1
    d = (cs - r) & M64 if r else 0
    far = 2 * ns * SUB_BYTES
    return min(d, far), (q + (1 if r else 0)) & M64, fixes


def tile_info(T, ns, n, cs):
    """tile_info<NS>(p, T) with the parameters run_byte_pass passes for a buffer of n bytes."""
    cs_subs, cs_subs_magic, cs_magic = byte_pass_geometry(n, cs)
    if cs_subs:
        return tile_info_subs(ns * T, ns, cs_subs, cs_subs_magic)
    return tile_info_bytes(T, ns, cs, cs_magic)
