"""numpy restatement of mtsv_batch_take_reads (k_compact.hip): the reads of a batch that a boolean mask keeps, packed in
order, and the composition of read maps along a chain of such steps.  No device, no library."""
import numpy as np

CODE = np.full(256, 4, dtype=np.uint8)       # src/binner.rs:88-100: A/a C/c G/g T/t -> 0..3, any other byte -> N (4)
for _i, _c in enumerate(b"ACGT"):
    CODE[_c] = CODE[_c + 32] = _i


def normalise(bases):
    """the byte codes the kernels see for raw read bytes"""
    return CODE[np.asarray(bases, dtype=np.uint8)]


def compact(codes, off, keep_mask, src_map=None):
    """(codes, offsets from 0, read map) of the reads i with keep_mask[i], in order.  off has n + 1 entries and may start
    anywhere; src_map (the map of the batch itself, when it came out of an earlier step) defaults to the identity."""
    codes = np.asarray(codes, dtype=np.uint8)
    off = np.asarray(off, dtype=np.uint64).astype(np.int64)
    keep_mask = np.asarray(keep_mask, dtype=bool)
    n = len(off) - 1
    assert len(keep_mask) == n
    idx = np.nonzero(keep_mask)[0]
    lens = (off[1:] - off[:-1])[idx]
    out_off = np.zeros(len(idx) + 1, dtype=np.uint64)
    np.cumsum(lens, out=out_off[1:])
    out = np.zeros(int(out_off[-1]), dtype=np.uint8)
    for j, i in enumerate(idx):
        out[int(out_off[j]):int(out_off[j + 1])] = codes[off[i]:off[i + 1]]
    src_map = np.arange(n, dtype=np.uint64) if src_map is None else np.asarray(src_map, dtype=np.uint64)
    assert len(src_map) == n
    return out, out_off, src_map[idx]


def compose(first, second):
    """the map of a batch that was cut out of a batch with the map `first` by a step whose own map is `second`"""
    return np.asarray(first, dtype=np.uint64)[np.asarray(second, dtype=np.int64)]


def keep_mask(flags, keep_matched):
    flags = np.asarray(flags, dtype=bool)
    return flags if keep_matched else ~flags
