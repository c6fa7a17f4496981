// pair.hip -- mtsv_fold_pair (include/mtsv_amd.h): the records of the two mates of every read pair of a fold joined into one
// record per (pair, TaxID), by the kernels of k_pair.hip.  The host reads the counters twice: before anything is written to
// the output fold (records with an edit of 2^31 or more, the size of the output), and after (the stats).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>

#include "fold.hpp"
#include "pair.hpp"

namespace mtsv {

PairState::PairState(int device_, hipStream_t stream_) : device(device_), stream(stream_) {
    timing = getenv("MTSV_PAIR_TIMING") != nullptr;
    HIP_CHECK(hipSetDevice(device));
    ev.create();
}

PairState::~PairState() {
    if (hipSetDevice(device) != hipSuccess) (void)hipGetLastError();
    if (stream) (void)hipStreamSynchronize(stream);
}

void Fold::pair(int mode, uint32_t max_insert, uint32_t unpaired_edits, Fold* out, mtsv_pair_stats* stats, float* device_ms) {
    if (!out) throw std::runtime_error("arg: no output fold");
    if (out == this) throw std::runtime_error("arg: the output fold is the fold itself");
    if (out->device != device) throw std::runtime_error("arg: the output fold is on device " + std::to_string(out->device) + ", the fold on device " + std::to_string(device));
    if (out->grain != MTSV_GRAIN_TAXID) throw std::runtime_error("arg: the grain of the output fold is not MTSV_GRAIN_TAXID: a pair's record is (pair, TaxID, edit)");
    if (mode != MTSV_PAIR_BOTH && mode != MTSV_PAIR_EITHER && mode != MTSV_PAIR_PROPER) throw std::runtime_error("arg: bad pair mode " + std::to_string(mode));
    if (n_reads & 1) throw std::runtime_error("arg: the fold numbers " + std::to_string(n_reads) + " reads, an odd number: reads 2p and 2p + 1 are the mates of pair p");
    if (mode == MTSV_PAIR_PROPER && grain != MTSV_GRAIN_LONG)
        throw std::runtime_error("arg: MTSV_PAIR_PROPER needs a fold at MTSV_GRAIN_LONG (the mates' GIs and offsets), this one's grain is " + std::to_string(grain));
    if (mode == MTSV_PAIR_EITHER && unpaired_edits >= 0x80000000u)
        throw std::runtime_error("arg: unpaired_edits of " + std::to_string(unpaired_edits) + ", 2^31 or more");
    if (n_reads >= (1ull << 32)) throw std::runtime_error("limit: a fold of " + std::to_string(n_reads) + " reads, 2^32 or more, in mtsv_fold_pair");
    const uint64_t P = n_reads / 2;
    if (device_ms) *device_ms = 0;
    if (stats) *stats = mtsv_pair_stats{P, 0, 0, 0, 0};
    if (!n) {  // (no read has a record: nothing is allocated or launched)
        out->reset(P);
        out->taxa = taxa;
        return;
    }
    HIP_CHECK(hipSetDevice(device));
    if (!pair_state) pair_state.reset(new PairState(device, stream));
    PairState& S = *pair_state;
    const double t0 = S.timing ? now_ms() : 0;
    const bool either = mode == MTSV_PAIR_EITHER;
    const uint32_t N = (uint32_t)n;  // (a fold holds fewer than 2^32 records)
    const uint32_t tiles = pair_tiles(n, pair_tile);
    // ---- room: by record and by run, of which there are at most as many ----
    S.d_off.room(stream, n_reads + 1, "the reads' first records");
    S.d_val.room(stream, n, "the records' values");
    S.d_add.room(stream, n, "the runs' partners");
    S.d_list.room(stream, n + 1, "the work list");
    if (either) S.d_pos_b.room(stream, n + 1, "the places in the second list");
    S.d_m.room(stream, n, "the runs' minima");
    S.d_slot.room(stream, n, "the runs' keys");
    S.d_tile_cnt.room(stream, std::max<uint64_t>(tiles, fold_tiles(n, tile)), "the tiles' heads");
    S.d_tile_off.room(stream, std::max<uint64_t>(tiles, fold_tiles(n, tile)) + 1, "the tiles' offsets");
    S.d_sums.room(stream, (uint64_t)scan_tiles(N) + 1, "the scans' sums");
    S.d_ctr.room(stream, kPairCounters + 4, "the counters");
    uint64_t *d_n_slots = S.d_ctr.p + kPairCounters, *d_n_a = d_n_slots + 1, *d_n_b = d_n_slots + 2, *d_n_merged = d_n_slots + 3;
    uint32_t *flag_a = S.d_val.p, *flag_b = either ? S.d_add.p : nullptr;  // (val and add are read for the last time by the minimum)
    uint32_t *pos_a = S.d_list.p, *pos_b = either ? S.d_pos_b.p : nullptr;  // (the list by the wavefront tier)
    // ---- join and reduce: nothing of the output fold is touched ----
    HIP_CHECK(hipMemsetAsync(S.d_ctr.p, 0, (kPairCounters + 4) * sizeof(uint64_t), stream));
    HIP_CHECK(hipMemsetAsync(S.d_m.p, 0xff, n * sizeof(uint32_t), stream));
    HIP_CHECK(hipEventRecord(S.ev[0], stream));
    launch_pair_bounds(stream, grain, d_rec[cur].p, N, n_reads, S.d_off.p);
    HIP_CHECK(hipEventRecord(S.ev[1], stream));
    launch_pair_join(stream, grain, mode, d_rec[cur].p, N, n_reads, S.d_off.p, max_insert, unpaired_edits, pair_lane_max, S.d_val.p, S.d_add.p, S.d_list.p,
                     S.d_ctr.p);
    HIP_CHECK(hipEventRecord(S.ev[2], stream));
    launch_pair_wave(stream, grain, mode, d_rec[cur].p, N, n_reads, S.d_off.p, max_insert, S.d_list.p, S.d_ctr.p, S.d_val.p, S.d_add.p);
    HIP_CHECK(hipEventRecord(S.ev[3], stream));
    launch_pair_heads(stream, grain, d_rec[cur].p, N, pair_tile, S.d_tile_cnt.p);
    launch_scan(stream, S.d_tile_cnt.p, tiles, S.d_sums.p, d_n_slots, S.d_tile_off.p);
    launch_pair_min(stream, grain, d_rec[cur].p, N, pair_tile, S.d_tile_off.p, S.d_val.p, S.d_add.p, N, S.d_m.p, S.d_slot.p);
    launch_pair_flags(stream, d_n_slots, N, S.d_slot.p, S.d_m.p, flag_a, flag_b);
    launch_scan(stream, flag_a, N, S.d_sums.p, d_n_a, pos_a);
    if (either) launch_scan(stream, flag_b, N, S.d_sums.p, d_n_b, pos_b);
    HIP_CHECK(hipEventRecord(S.ev[4], stream));
    uint64_t ctr[kPairCounters + 4] = {};
    HIP_CHECK(hipMemcpyAsync(ctr, S.d_ctr.p, sizeof ctr, hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    HIP_CHECK(hipGetLastError());
    const uint64_t n_slots = ctr[kPairCounters], n_a = ctr[kPairCounters + 1], n_b = ctr[kPairCounters + 2], total = n_a + n_b, n_listed = ctr[kPairCtrList];
    if (ctr[kPairCtrBadEdit])
        throw std::runtime_error("arg: " + std::to_string(ctr[kPairCtrBadEdit]) + " records of the fold carry an edit of 2^31 or more");
    if (ctr[kPairCtrBeyond])
        throw std::runtime_error("internal: " + std::to_string(ctr[kPairCtrBeyond]) + " records of the fold belong to reads numbered at or above its " + std::to_string(n_reads));
    if (!n_slots || n_slots > n || total > n_slots || n_listed > n)
        throw std::runtime_error("internal: " + std::to_string(n) + " records in " + std::to_string(n_slots) + " runs gave " + std::to_string(n_a) + " and " +
                                 std::to_string(n_b) + " records, " + std::to_string(n_listed) + " listed");
    if (total >= (1ull << 32)) throw std::runtime_error("limit: the pair fold would hold " + std::to_string(total) + " records, 2^32 or more");
    // ---- write: into the output fold's other array, or a new pair when it is too small; two lists are merged into it ----
    const bool merge = n_a && n_b;
    Staged st = total ? out->stage_write(total, "an output fold") : Staged{};  // (an error below frees a pair it holds: the output fold stays as it was)
    if (merge) S.d_lists.room(stream, total * sizeof(mtsv_assignment), "the two lists");
    uint8_t* list_a = merge ? S.d_lists.p : st.dst;
    uint8_t* list_b = merge ? S.d_lists.p + n_a * sizeof(mtsv_assignment) : st.dst;
    HIP_CHECK(hipEventRecord(S.ev[5], stream));
    if (total) launch_pair_write(stream, d_n_slots, N, S.d_slot.p, S.d_m.p, pos_a, pos_b, (uint32_t)n_a, (uint32_t)n_b, list_a, list_b);
    if (merge) {
        const uint32_t m_tiles = fold_tiles(total, tile);
        launch_fold_count(stream, MTSV_GRAIN_TAXID, list_a, (uint32_t)n_a, list_b, (uint32_t)n_b, tile, S.d_tile_cnt.p);
        launch_scan(stream, S.d_tile_cnt.p, m_tiles, S.d_sums.p, d_n_merged, S.d_tile_off.p);
        launch_fold_write(stream, MTSV_GRAIN_TAXID, list_a, (uint32_t)n_a, list_b, (uint32_t)n_b, tile, S.d_tile_off.p, st.dst);
    }
    HIP_CHECK(hipEventRecord(S.ev[6], stream));
    launch_pair_stats(stream, S.d_off.p, P, st.dst, (uint32_t)total, S.d_ctr.p);
    HIP_CHECK(hipEventRecord(S.ev[7], stream));
    HIP_CHECK(hipMemcpyAsync(ctr, S.d_ctr.p, sizeof ctr, hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    HIP_CHECK(hipGetLastError());
    if (merge && ctr[kPairCounters + 3] != total)
        throw std::runtime_error("internal: the merge of " + std::to_string(n_a) + " and " + std::to_string(n_b) + " records of disjoint keys counted " +
                                 std::to_string(ctr[kPairCounters + 3]));
    if (ctr[kPairCtrJoined] > total || ctr[kPairCtrBoth] + ctr[kPairCtrOne] > P)
        throw std::runtime_error("internal: " + std::to_string(ctr[kPairCtrJoined]) + " pairs joined in " + std::to_string(total) + " records, " +
                                 std::to_string(ctr[kPairCtrBoth]) + " + " + std::to_string(ctr[kPairCtrOne]) + " of " + std::to_string(P) + " pairs hit");
    float ms[6] = {0, 0, 0, 0, 0, 0};
    for (int k = 0; k < 4; k++) HIP_CHECK(hipEventElapsedTime(&ms[k], S.ev[k], S.ev[k + 1]));
    for (int k = 4; k < 6; k++) HIP_CHECK(hipEventElapsedTime(&ms[k], S.ev[k + 1], S.ev[k + 2]));
    // ---- nothing can fail from here ----
    if (total) out->commit(st, total);
    else out->reset(P);
    out->n_reads = P;
    out->taxa = taxa;
    if (stats) *stats = mtsv_pair_stats{P, ctr[kPairCtrBoth], ctr[kPairCtrOne], ctr[kPairCtrJoined], total};
    const float all_ms = ms[0] + ms[1] + ms[2] + ms[3] + ms[4] + ms[5];
    if (device_ms) *device_ms = all_ms;
    if (trace)
        fprintf(stderr, "[pair] mode %d, %llu records of %llu pairs in %llu runs, %llu on the work list (lane tier up to %u), tiles of %u -> %llu records: %.3f ms\n", mode,
                (unsigned long long)n, (unsigned long long)P, (unsigned long long)n_slots, (unsigned long long)n_listed, pair_lane_max, pair_tile,
                (unsigned long long)total, all_ms);
    // MTSV_PAIR_TIMING=1: where a call spends its time (tools/pair_ab.py reads this line)
    if (S.timing)
        fprintf(stderr, "[pair timing] mode %d records %llu pairs %llu runs %llu listed %llu out %llu; bounds %.3f ms, join %.3f ms, wave %.3f ms, reduce %.3f ms, "
                        "write %.3f ms, stats %.3f ms, call %.3f ms\n",
                mode, (unsigned long long)n, (unsigned long long)P, (unsigned long long)n_slots, (unsigned long long)n_listed, (unsigned long long)total, ms[0], ms[1],
                ms[2], ms[3], ms[4], ms[5], now_ms() - t0);
}

}  // namespace mtsv
