"""No GPU: a Python model of the coalescing walk of a strand's sorted seed hits (index.rs:445-485 as k_coalesce.hip
restates it) against the walk by runs that k_coalesce_heavy uses (walk_by_runs): the sorted hits are cut wherever the
serial walk cannot merge whatever came before -- at a hit that is not `ok`, behind one that is not `ok`, where the bin
changes, and (a cut the kernel may or may not make) where a window starts at or behind the largest window end since the
last cut -- and every piece is walked on its own from an empty state.  The candidates, in order of the hit at which their
segment ends, must be the serial walk's, candidate for candidate."""
import random

import pytest

RUN_MAX = 256  # k_coalesce.hip: kRunMax


def find_bin(bin_ends, site):
    """first bin whose end > site, clamped to the last bin (find_bin + the min() at its call sites)"""
    lo, hi = 0, len(bin_ends) - 1
    while lo < hi:
        mid = (lo + hi) // 2
        if bin_ends[mid] <= site:
            lo = mid + 1
        else:
            hi = mid
    return lo


def candidate_window(site, q, b_start, b_end, L, ED):
    """SeedHit::candidate_indices (index.rs:118-153) -> (ok, ws, we)"""
    so = q + ED
    s = b_start if (so > site or site - so < b_start) else site - so
    e = min(site + (L - q) + ED, b_end)
    return (not (s > e or e - s < L - ED)), s, e


def hit_records(hits, bins, L, ED):
    ends = [b[1] for b in bins]
    out = []
    for site, q in hits:
        b = find_bin(ends, site)
        ok, ws, we = candidate_window(site, q, bins[b][0], bins[b][1], L, ED)
        out.append((b, ok, ws, we))
    return out


def serial_walk(recs, min_seeds):
    """the walk as coalesce_big's one wavefront does it; candidates (s, e, n, b) in flush order"""
    out = []
    have, s, e, b, n = False, 0, 0, 0, 0
    for bi, oki, wsi, wei in recs:
        merge = have and oki and bi == b and ((s <= wsi < e) or (s < wei <= e))
        if merge:
            s, e, n = min(s, wsi), max(e, wei), n + 1
        else:
            if have and n >= min_seeds:
                out.append((s, e, n, b))
            have, s, e, b, n = oki, wsi, wei, bi, 1
    if have and n >= min_seeds:
        out.append((s, e, n, b))
    return out


def run_heads(recs, running_max):
    heads = []
    top = 0
    for i, (b, ok, ws, we) in enumerate(recs):
        head = i == 0 or not ok or not recs[i - 1][1] or b != recs[i - 1][0]
        if running_max and not head and ws >= top:
            head = True
        if head:
            top = 0
        top = max(top, we)
        heads.append(head)
    return heads


def walk_by_runs(recs, min_seeds, running_max=False, run_max=RUN_MAX):
    """-> (candidates in order of the hit their segment ends at, took_fallback)"""
    heads = run_heads(recs, running_max)
    starts = [i for i, h in enumerate(heads) if h] + [len(recs)]
    if any(b - a > run_max for a, b in zip(starts, starts[1:])):
        return serial_walk(recs, min_seeds), True
    kept = {}  # last hit of a kept segment -> its candidate
    for a, z in zip(starts, starts[1:]):  # every run on its own, in any order
        b, ok, s, e = recs[a]
        if not ok:
            assert z == a + 1
            continue
        n = 1
        for j in range(a + 1, z):
            _, okj, wsj, wej = recs[j]
            assert okj and recs[j][0] == b
            if (s <= wsj < e) or (s < wej <= e):
                s, e, n = min(s, wsj), max(e, wej), n + 1
            else:
                if n >= min_seeds:
                    kept[j - 1] = (s, e, n, b)
                s, e, n = wsj, wej, 1
        if n >= min_seeds:
            kept[z - 1] = (s, e, n, b)
    return [kept[i] for i in sorted(kept)], False


def random_bins(rng, n_bins, small=False):
    bins, at = [], 0
    for _ in range(n_bins):
        ln = rng.randrange(20, 200) if small and rng.random() < 0.3 else rng.randrange(300, 5000)
        bins.append((at, at + ln))
        at += ln
    return bins


def random_strand(rng, bins, n_hits, L, K=18, G=15, clustered=0.7):
    """sorted (site, q) hits: clusters on a few diagonals (they merge), hits at bin edges (clamped windows of other
    lengths, windows that are not ok), and strays"""
    n = bins[-1][1]
    qs = list(range(0, L - K + 1, G))
    hits = []
    while len(hits) < n_hits:
        r = rng.random()
        if r < clustered:
            b = rng.choice(bins)
            origin = rng.randrange(b[0] - 30, b[1] + 30)
            for q in rng.sample(qs, rng.randrange(1, len(qs) + 1)):
                site = origin + q + rng.choice((0, 0, 0, 1, -2, 7))
                if 0 <= site < n:
                    hits.append((site, q))
        elif r < 0.85:
            b = rng.choice(bins)
            site = rng.choice((b[0], b[0] + 1, b[1] - 1, b[1] - K, b[0] + rng.randrange(0, 40)))
            if 0 <= site < n:
                hits.append((site, rng.choice(qs)))
        else:
            hits.append((rng.randrange(n), rng.choice(qs)))
    hits = hits[:n_hits]
    hits.sort()
    return hits


def check(recs, min_seeds, expect_fallback=None):
    want = serial_walk(recs, min_seeds)
    for running_max in (False, True):
        got, fell_back = walk_by_runs(recs, min_seeds, running_max)
        assert got == want, (running_max, min_seeds, len(recs))
        if expect_fallback is not None and not running_max:
            assert fell_back == expect_fallback
    return want


@pytest.mark.parametrize("n_bins", [1, 2, 40, 400])
def test_walk_by_runs_equals_the_serial_walk(n_bins):
    rng = random.Random(1000 + n_bins)
    n_cands = n_not_ok = n_lengths = 0
    for it in range(400):
        L = rng.choice((60, 100, 150, 253))
        ED = -(-L * 13 // 100)
        bins = random_bins(rng, n_bins, small=it % 3 == 0)
        hits = random_strand(rng, bins, rng.randrange(65, 500), L)
        recs = hit_records(hits, bins, L, ED)
        n_not_ok += sum(not r[1] for r in recs)
        n_lengths += len({r[3] - r[2] for r in recs if r[1]}) > 1
        for min_seeds in (1, 2, 3):
            n_cands += len(check(recs, min_seeds))
    assert n_cands > 1000
    assert n_lengths > 100, "windows clamped at bin edges: lengths must differ"
    if n_bins > 1:
        assert n_not_ok > 0, "small bins: some windows must fail candidate_indices"


def test_two_bins_with_the_boundary_inside_a_window():
    """hits on both sides of a bin boundary, closer than a window: they must not merge across it"""
    rng = random.Random(5)
    L, ED = 150, 20
    bins = [(0, 5000), (5000, 9000)]
    for it in range(300):
        hits = sorted((5000 + rng.randrange(-160, 160), rng.choice(range(0, 133, 15))) for _ in range(rng.randrange(65, 300)))
        recs = hit_records(hits, bins, L, ED)
        assert {r[0] for r in recs} == {0, 1}
        for min_seeds in (1, 2, 3):
            for c in check(recs, min_seeds):
                assert bins[c[3]][0] <= c[0] and c[1] <= bins[c[3]][1]


def test_one_bin_tandem_repeat_takes_the_fallback():
    """every hit ok and in one bin: one run, longer than a thread walks -- the wavefront walk does the strand"""
    rng = random.Random(6)
    L, ED = 150, 20
    bins = [(0, 200000)]
    for n_hits, fallback in ((RUN_MAX, False), (RUN_MAX + 1, True), (2048, True)):
        hits = sorted((1000 + 97 * rng.randrange(0, 1500) + q, q) for q in rng.choices(range(0, 133, 15), k=n_hits))
        recs = hit_records(hits, bins, L, ED)
        assert all(r[1] for r in recs)
        for min_seeds in (1, 2, 3):
            check(recs, min_seeds, expect_fallback=fallback)


def test_a_cut_is_never_a_merge():
    """the argument itself, hit by hit: at every cut of either kind the serial walk does not merge"""
    rng = random.Random(7)
    n_cuts = 0
    for it in range(300):
        L = rng.choice((100, 150))
        ED = -(-L * 13 // 100)
        bins = random_bins(rng, rng.choice((1, 3, 50)), small=True)
        recs = hit_records(random_strand(rng, bins, rng.randrange(65, 400), L), bins, L, ED)
        heads = run_heads(recs, running_max=True)
        have, s, e, b = False, 0, 0, 0
        for (bi, oki, wsi, wei), head in zip(recs, heads):
            merge = have and oki and bi == b and ((s <= wsi < e) or (s < wei <= e))
            assert not (head and merge)
            n_cuts += head
            if merge:
                s, e = min(s, wsi), max(e, wei)
            else:
                have, s, e, b = oki, wsi, wei, bi
    assert n_cuts > 10000
