"""The cases of the deep-read tests hold what they claim (deep_cases.py), from the CPU oracle alone: per case the oracle's
hits per chunk, merged by chunk_merge_ref.merge_hits, put the deep reads on both sides of every edge test_deep_reads.py is
about -- before anything goes near a GPU.

  case        sources           hits of a deep read    what it reaches
  two_trips   5 full            640                    N = 1024: the second trip of the sorting network, LDS tier, all grains
  wide_edge   16 full + unit    2048 and 2049          LDS edge of the wide grains at the default threshold
  taxid_edge  32 full + unit    4096 and 4097          LDS edge of the taxid grain
  ragged      40 full           5120                   global tier, N = 8192 with 3072 skipped upper indexes
  full_house  64 full           8192                   the source limit, N = n = 8192
  moved_edge  8 full            1024                   n = MTSV_COLLAPSE_LDS_MAX = 1024 exactly
  one_pass    wide_chunk        > 512, both strands    the layout of a pass, not the collector's

by_edit and edit_later (one long key with two edits) exist only in merged lists -- one index never returns a long key
twice with different edits -- so one_pass is asked for the other four census counts."""
import numpy as np
import pytest

import deep_cases as D
import grain_cases as G
import grain_ref as GR

LDS_KEYS, LDS_KEYS_WIDE, THREADS, FOLD_TILE = 4096, 2048, 256, 1024   # k_collapse.hip, k_fold.hip


def network(n):
    """(N, pairs a thread of the workgroup visits per step, upper indexes past the end) of block_bitonic on n keys"""
    N = 1
    while N < n:
        N <<= 1
    return N, max(1, (N >> 1) // THREADS), N - n


def kinds_of(name):
    return [i for i, k in enumerate(D.KINDS) if k == name]


def test_reads_are_what_the_cases_need():
    assert len(D.READS) == D.N_DEEP + D.N_BG + D.N_NONE and len(D.DEEP) == D.N_DEEP
    assert len(kinds_of("in")) == len(kinds_of("out")) == D.N_DEEP // 2
    groups = [i // 64 for i in D.DEEP]
    assert len(set(groups)) > 1 and max(groups.count(g) for g in set(groups)) > 1
    assert D.SEG != G.database()[2]                              # a segment of its own, not the per-chunk seed's
    taxa = {G.tax_of(t) for t in range(D.S_FULL)}
    assert len(taxa) == D.H // 2 and any(t >> 31 for t in taxa) and any(G.gi_of(t) >> 31 for t in range(D.S_FULL))
    # chunks 2p and 2p + 1: the even sequences share their flanks and differ in their substitutions, the odd ones do not
    a, b, c = D.full_chunk(2), D.full_chunk(3), D.full_chunk(4)
    for t in (30, 31):
        ea, eb, ec = a[t][2], b[t][2], c[t][2]
        assert ea != eb and ea != ec
        assert (len(ea) == len(eb) and sum(x != y for x, y in zip(ea, eb)) <= 16) == (t % 2 == 0)
        assert sum(x != y for x, y in zip(ea, ec)) > 100


@pytest.mark.parametrize("case", list(D.CASES))
def test_case_holds_what_it_claims(case):
    full, unit, lds_max = D.CASES[case]
    parts = D.parts(case)
    hits = D.merged(case)
    assert len(hits) == sum(len(p) for p in parts)
    per_read = D.per_read(hits)
    assert (per_read[kinds_of("bg")] == 1).all() and (per_read[kinds_of("none")] == 0).all()
    c = G.census(hits)
    assert c["tax31"] and c["gi31"] and c["winner_later"] and c["offset_decides"], c
    if case == "one_pass":
        deep = per_read[D.DEEP]
        assert (deep > 512).all() and (deep <= LDS_KEYS_WIDE).all()
        for r in D.DEEP:
            fwd, rev = D.strand_counts(hits, r)
            assert fwd > 0 and rev > 0 and fwd + rev == per_read[r] > 512
        assert all(network(int(n))[1] == 2 for n in deep)        # N = 1024: two trips
        return
    for p, key in zip(parts, D.chunk_keys(case)):                # H per deep read and full chunk, 1 / 0 in the unit chunk
        pr = D.per_read(p)
        if key[0] == "full":
            assert (pr[D.DEEP] == D.H).all()
        else:
            assert (pr[kinds_of("in")] == 1).all() and (pr[kinds_of("out")] == 0).all() and pr.sum() == D.N_DEEP // 2
    want = D.want_counts(case)
    for kind in ("in", "out"):
        assert (per_read[kinds_of(kind)] == want[kind]).all(), (kind, want[kind], per_read[kinds_of(kind)])
    assert c["by_edit"] and c["edit_later"], c
    assert c["group_max"] >= full, c
    n_in, n_out = want["in"], want["out"]
    if case == "two_trips":
        assert n_in == n_out == 640 and network(640) == (1024, 2, 384) and 640 <= LDS_KEYS_WIDE
    elif case == "wide_edge":
        assert (n_out, n_in) == (LDS_KEYS_WIDE, LDS_KEYS_WIDE + 1) and n_in <= LDS_KEYS
    elif case == "taxid_edge":
        assert (n_out, n_in) == (LDS_KEYS, LDS_KEYS + 1)
    elif case == "ragged":
        assert n_in == n_out == 5120 > LDS_KEYS and network(5120) == (8192, 16, 3072)
    elif case == "full_house":
        assert full == D.N_FULL == 64 and n_in == n_out == 8192 and network(8192) == (8192, 16, 0)
        longs = GR.collapse_long(hits)
        r = D.DEEP[0]
        assert sum(1 for rec in longs if rec[0] == r) > LDS_KEYS  # more than 4096 distinct long keys in one read
        assert 8192 // FOLD_TILE == 8
    elif case == "moved_edge":
        assert n_in == n_out == lds_max == 1024
