"""Plain-Python restatements of what an upload leaves in HBM (dev_layout.hpp, dev_index.hip), computed from the bytes of
the index file alone: the rank blocks, the text codes, the scalars of the header and the small arrays.  With a reader of
the bincode file (mgindex.hpp) that also knows where every Occ checkpoint lies, so that a test can patch one.

Nothing here is shared with the code under test; test_device_pack_cpu.py pins blocks() by brute force."""
import struct

CODE = {ord("A"): 0, ord("C"): 1, ord("G"): 2, ord("T"): 3, ord("N"): 4, ord("$"): 5}
SYMS = "ACGTN$"
BLOCK_ROWS = 128

# the rungs of helpers.RUNGS the pack is tested on: block and default-tile (64 blocks = 8192 rows) edges and the all-padding
# extra block of n % 128 == 0; the sentinel at residues 0/1/63/64/127 and in the first and last block; Occ intervals 3, 128,
# 1 and beyond n; a long N run; thousands of bins
RUNG_NAMES = tuple("random-%d" % n for n in (1, 2, 3, 127, 128, 129, 255, 256, 257, 8191, 8192, 8193, 65537, 524161)) + \
    tuple("sentinel-" + t for t in ("res0", "res1", "res63", "res64", "res127", "first_block", "last_block")) + \
    ("A-129", "ACG-4096", "nrun-20000", "tinybins-117001", "sampling-257-k1-s1", "sampling-257-k262-s258", "sampling-4097-k4102-s32")


class IndexFile:
    """text, bins [(gi, tax_id, start, end)], bwt, less [118], occ {symbol: [checkpoints]}, k, sample, s -- and
    occ_offset(symbol, j): the byte of the file at which the u64 occ[symbol][j] begins"""

    def __init__(self, path):
        raw = open(path, "rb").read()
        at = 0

        def u64():
            nonlocal at
            v = struct.unpack_from("<Q", raw, at)[0]
            at += 8
            return v

        def take(n):
            nonlocal at
            b = raw[at:at + n]
            assert len(b) == n
            at += n
            return b

        self.text = take(u64())
        self.bins = [struct.unpack_from("<IIQQ", take(24)) for _ in range(u64())]
        self.bwt = take(u64())
        self.less = list(struct.unpack("<%dQ" % 118, take(8 * u64())))
        self.occ, self._occ_at = {}, {}
        n_outer = u64()
        assert n_outer == 117 and len(self.less) == 118
        for a in range(n_outer):
            ln = u64()
            if chr(a) in SYMS:
                self._occ_at[chr(a)] = at
                self.occ[chr(a)] = list(struct.unpack_from("<%dQ" % ln, raw, at))
            at += 8 * ln
        self.k = struct.unpack_from("<I", raw, at)[0]
        at += 4
        ns = u64()
        self.sample = list(struct.unpack_from("<%dQ" % ns, raw, at))
        at += 8 * ns
        self.s = u64()
        take(16 * u64())          # extra_rows
        assert raw[at:at + 1] == b"$" and at + 1 == len(raw)
        self.n = len(self.text)
        assert len(self.bwt) == self.n

    def occ_offset(self, sym, j):
        assert 0 <= j < len(self.occ[sym])
        return self._occ_at[sym] + 8 * j


def n_blocks(n):
    return (n >> 7) + 1


def blocks(bwt):
    """the RankBlock array: per 128 rows cnt[4] (A, C, G, T in the rows before the block), then the planes p0[2], p1[2], p2[2]
    of the rows' 3-bit codes; rows at and beyond n hold 7"""
    n = len(bwt)
    out = bytearray()
    cnt = [0, 0, 0, 0]
    for b in range(n_blocks(n)):
        planes = [0, 0, 0]
        seen = list(cnt)
        for o in range(BLOCK_ROWS):
            i = b * BLOCK_ROWS + o
            code = CODE[bwt[i]] if i < n else 7
            if code < 4:
                cnt[code] += 1
            for p in range(3):
                planes[p] |= ((code >> p) & 1) << o
        out += struct.pack("<4I", *seen)
        for p in range(3):
            out += struct.pack("<2Q", planes[p] & (2 ** 64 - 1), planes[p] >> 64)
    return bytes(out)


def codes(text):
    n = len(text)
    return bytes(CODE.get(c, 7) for c in text) + b"\x07" * ((n + 15) // 16 * 16 + 32 - n)


def bin_lut(f):
    shift = 0
    while (f.n >> shift) > 65536:
        shift += 1
    ends = [b[3] for b in f.bins]
    lut, b = [], 0
    for k in range((f.n >> shift) + 2):
        while b + 1 < len(ends) and ends[b] <= (k << shift):
            b += 1
        lut.append(b)
    return shift, lut


def header(f):
    """the scalars of mtsv_device_header that the file decides (kmer_k, sa_full, device_bytes depend on flags and device)"""
    shift, _ = bin_lut(f)
    pow2 = 0xFFFFFFFF
    for sh in range(32):
        if 1 << sh == f.s:
            pow2 = sh
    return dict(n=f.n, n_blocks=n_blocks(f.n), C=[f.less[ord(c)] for c in "ACGTN"], sentinel_row=f.bwt.index(b"$"), sa_s=f.s,
                sa_pow2_shift=pow2, n_bins=len(f.bins), bin_lut_shift=shift)


def small_parts(f):
    """SA_SAMPLE, BINS, BIN_END, BIN_LUT as the device holds them"""
    _, lut = bin_lut(f)
    return dict(sa_sample=struct.pack("<%dI" % len(f.sample), *f.sample),
                bins=b"".join(struct.pack("<4I", start, end, tax, gi) for gi, tax, start, end in f.bins),
                bin_end=struct.pack("<%dI" % len(f.bins), *[b[3] for b in f.bins]),
                bin_lut=struct.pack("<%dI" % len(lut), *lut))
