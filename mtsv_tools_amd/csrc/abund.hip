// abund.hip -- mtsv_fold_abundance (include/mtsv_amd.h): the entry list of a fold's records, built once per call, and the
// iterations of k_abund.hip over it.  What comes down is counters, 8 bytes per iteration and, at the end, 20 bytes per TaxID
// of the union; the assigned records stay in HBM, in the output fold.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>

#include "abund.hpp"
#include "fold.hpp"

namespace mtsv {

AbundState::AbundState(int device_, hipStream_t stream_) : device(device_), stream(stream_) {
    timing = getenv("MTSV_ABUND_TIMING") != nullptr;
    HIP_CHECK(hipSetDevice(device));
    int n_cu = 0;
    HIP_CHECK(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device));
    cus = (uint32_t)std::max(n_cu, 1);
    ev.create();
}

AbundState::~AbundState() {
    if (hipSetDevice(device) != hipSuccess) (void)hipGetLastError();
    if (stream) (void)hipStreamSynchronize(stream);
}

void Fold::abundance(const uint32_t* w, uint32_t n_w, uint32_t edit_slack, uint32_t max_iters, uint64_t tol, Fold* out, std::vector<mtsv_abundance_row>* rows,
                     mtsv_abundance_info* info, float* device_ms) {
    if (!w) throw std::runtime_error("arg: null weight table");
    if (n_w < 1 || n_w > 255) throw std::runtime_error("arg: a weight table of " + std::to_string(n_w) + " entries (1 .. 255)");
    if (out == this) throw std::runtime_error("arg: the output fold is the fold itself");
    if (out && out->device != device) throw std::runtime_error("arg: the output fold is on device " + std::to_string(out->device) + ", the fold on device " + std::to_string(device));
    if (out && out->grain != MTSV_GRAIN_TAXID) throw std::runtime_error("arg: the grain of the output fold is not MTSV_GRAIN_TAXID: a read's assignment is one (read, TaxID, edit) record");
    if (rows) rows->clear();
    if (info) *info = mtsv_abundance_info{};
    if (device_ms) *device_ms = 0;
    if (!n) {  // (no read has a record: nothing is allocated or launched)
        if (out) out->reset(n_reads);
        return;
    }
    HIP_CHECK(hipSetDevice(device));
    if (!abund_state) abund_state.reset(new AbundState(device, stream));
    AbundState& S = *abund_state;
    const double t0 = S.timing ? now_ms() : 0;
    // ---- the reads with a record and the (read, TaxID) runs ----
    const uint32_t tiles = abund_tiles(n, abund_tile), U = (uint32_t)taxa.size();
    constexpr uint32_t kTotals = kAbundCounters, kL1 = kAbundCounters + 3, kCtrAll = kAbundCounters + 4;
    S.d_tile.room(stream, 4ull * tiles + 2, "the tiles' heads");
    S.d_ctr.room(stream, kCtrAll, "the counters");
    uint32_t *d_cnt_r = S.d_tile.p, *d_cnt_p = d_cnt_r + tiles, *d_off_r = d_cnt_p + tiles, *d_off_p = d_off_r + tiles + 1;
    S.d_sums.room(stream, (uint64_t)scan_tiles(tiles) + 1, "the scans' sums");
    uint64_t ctr[kCtrAll] = {};
    HIP_CHECK(hipMemsetAsync(S.d_ctr.p, 0, sizeof ctr, stream));
    HIP_CHECK(hipEventRecord(S.ev[0], stream));
    launch_abund_heads(stream, grain, d_rec[cur].p, (uint32_t)n, abund_tile, d_cnt_r, d_cnt_p);
    launch_scan(stream, d_cnt_r, tiles, S.d_sums.p, S.d_ctr.p + kTotals, d_off_r);
    launch_scan(stream, d_cnt_p, tiles, S.d_sums.p, S.d_ctr.p + kTotals + 1, d_off_p);
    HIP_CHECK(hipEventRecord(S.ev[1], stream));
    HIP_CHECK(hipMemcpyAsync(ctr, S.d_ctr.p, sizeof ctr, hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    HIP_CHECK(hipGetLastError());
    const uint64_t R = ctr[kTotals], P = ctr[kTotals + 1];
    if (!R || R > P || P > n) throw std::runtime_error("internal: " + std::to_string(n) + " records of " + std::to_string(P) + " runs of " + std::to_string(R) + " reads");
    if (R >= (1ull << 31)) throw std::runtime_error("limit: " + std::to_string(R) + " reads with a record, 2^31 or more");
    // ---- room; whatever fails from here to the commit leaves both folds as they were ----
    S.d_sums.room(stream, (uint64_t)scan_tiles((uint32_t)P) + 1, "the scans' sums");
    S.d_read64.room(stream, R, "the reads' numbers");
    S.d_read32.room(stream, 4 * R + 1, "the reads' offsets");
    S.d_run32.room(stream, 5 * P + 1, "the runs");
    S.d_ent32.room(stream, 2 * P, "the abundance entries");
    S.d_ent8.room(stream, P, "the abundance entries");
    S.d_tax32.room(stream, 4ull * U + 256, "the taxa's counts");
    S.d_mass.room(stream, 2ull * U, "the abundance masses");
    if (!out) S.d_out.room(stream, R * sizeof(mtsv_assignment), "the reads' records");
    Staged st = out ? out->stage_write(R, "an output fold") : Staged{};  // (an error below frees a pair it holds)
    uint8_t* dst = out ? st.dst : S.d_out.p;
    uint32_t *d_m = S.d_read32.p, *d_read_first = d_m + R, *d_list = d_read_first + R, *d_read_off = d_list + R;
    uint32_t *d_e_run = S.d_run32.p, *d_run_tax = d_e_run + P, *d_run_read = d_run_tax + P, *d_flag = d_run_read + P, *d_off = d_flag + P;
    uint32_t *d_ent_slot = S.d_ent32.p, *d_ent_e = d_ent_slot + P;
    uint32_t *d_u_tax = S.d_tax32.p, *d_any = d_u_tax + U, *d_uniq = d_any + U, *d_assigned = d_uniq + U, *d_w = d_assigned + U;
    uint64_t *d_mass = S.d_mass.p, *d_next = d_mass + U;
    if (U) HIP_CHECK(hipMemcpyAsync(d_u_tax, taxa.data(), (size_t)U * 4, hipMemcpyHostToDevice, stream));
    HIP_CHECK(hipMemcpyAsync(d_w, w, (size_t)n_w * 4, hipMemcpyHostToDevice, stream));
    HIP_CHECK(hipMemsetAsync(d_m, 0xff, R * 4, stream));
    HIP_CHECK(hipMemsetAsync(d_e_run, 0xff, P * 4, stream));
    if (U) HIP_CHECK(hipMemsetAsync(d_any, 0, 3ull * U * 4, stream));  // (any, uniq, assigned)
    HIP_CHECK(hipEventRecord(S.ev[2], stream));
    launch_abund_min(stream, grain, d_rec[cur].p, (uint32_t)n, abund_tile, d_off_r, d_off_p, (uint32_t)R, (uint32_t)P, d_m, d_e_run, S.d_read64.p, d_read_first,
                     d_run_tax, d_run_read);
    launch_abund_flag(stream, (uint32_t)P, d_e_run, d_m, d_run_read, edit_slack, d_flag);
    launch_scan(stream, d_flag, (uint32_t)P, S.d_sums.p, S.d_ctr.p + kTotals + 2, d_off);
    launch_abund_write(stream, (uint32_t)R, (uint32_t)P, d_off, d_e_run, d_m, d_run_tax, d_run_read, d_read_first, d_u_tax, U, n_w, abund_lane_max, d_read_off,
                       d_ent_slot, S.d_ent8.p, d_ent_e, d_any, d_uniq, d_list, S.d_ctr.p);
    launch_abund_init(stream, U, d_any, abund_start_mass, d_mass, d_next);
    HIP_CHECK(hipEventRecord(S.ev[3], stream));
    HIP_CHECK(hipMemcpyAsync(ctr, S.d_ctr.p, sizeof ctr, hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    HIP_CHECK(hipGetLastError());
    const uint64_t E = ctr[kTotals + 2], n_list = ctr[kAbundCtrList];
    if (ctr[kAbundCtrMissing])
        throw std::runtime_error("internal: " + std::to_string(ctr[kAbundCtrMissing]) + " entries of the fold carry a TaxID that is not in its union of " + std::to_string(U) + " TaxIDs");
    if (ctr[kAbundCtrLong])
        throw std::runtime_error("limit: " + std::to_string(ctr[kAbundCtrLong]) + " reads with 65536 or more entering TaxIDs");
    if (E < R || E > P || n_list > R)
        throw std::runtime_error("internal: " + std::to_string(E) + " entries of " + std::to_string(R) + " reads in " + std::to_string(P) + " runs, " + std::to_string(n_list) + " listed");
    float ms_prepare[2] = {0, 0}, ms_step = 0, ms_delta = 0, ms_final = 0;
    HIP_CHECK(hipEventElapsedTime(&ms_prepare[0], S.ev[0], S.ev[1]));
    HIP_CHECK(hipEventElapsedTime(&ms_prepare[1], S.ev[2], S.ev[3]));
    // ---- the iterations: the host reads L1, 8 bytes, after each ----
    const bool dense = U <= abund_dense_max;
    const uint64_t work = std::max<uint64_t>(R, n_list * 64);
    // (dense: 64 KiB of LDS at the most, two workgroups per CU; else as many as a CU holds of 256 lanes)
    const uint32_t blocks = (uint32_t)std::min<uint64_t>(std::max<uint64_t>((work + 255) / 256, 1), (uint64_t)S.cus * (dense ? 2 : 8));
    const AbundEntries en{(uint32_t)R, (uint32_t)n_list, abund_lane_max, U, d_read_off, d_ent_slot, d_list, d_w, S.d_ent8.p};
    uint32_t iterations = 0, converged = 0;
    uint64_t l1 = 0;
    while (iterations < max_iters) {
        float a = 0, b = 0;
        HIP_CHECK(hipMemsetAsync(S.d_ctr.p + kL1, 0, sizeof(uint64_t), stream));
        HIP_CHECK(hipEventRecord(S.ev[4], stream));
        launch_abund_step(stream, blocks, dense, en, d_mass, d_next);
        HIP_CHECK(hipEventRecord(S.ev[5], stream));
        launch_abund_delta(stream, U, d_mass, d_next, S.d_ctr.p + kL1);
        HIP_CHECK(hipEventRecord(S.ev[6], stream));
        HIP_CHECK(hipMemcpyAsync(&l1, S.d_ctr.p + kL1, sizeof l1, hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipEventElapsedTime(&a, S.ev[4], S.ev[5]));
        HIP_CHECK(hipEventElapsedTime(&b, S.ev[5], S.ev[6]));
        ms_step += a;
        ms_delta += b;
        iterations++;
        if (l1 <= tol) {
            converged = 1;
            break;
        }
    }
    // ---- the hard assignment under the final masses ----
    std::vector<uint64_t> mass(U);
    std::vector<uint32_t> counts(3ull * U);
    HIP_CHECK(hipEventRecord(S.ev[7], stream));
    launch_abund_final(stream, blocks, en, d_mass, d_ent_e, S.d_read64.p, d_u_tax, dst, d_assigned);
    HIP_CHECK(hipEventRecord(S.ev[8], stream));
    if (U) {
        HIP_CHECK(hipMemcpyAsync(mass.data(), d_mass, (size_t)U * 8, hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipMemcpyAsync(counts.data(), d_any, 3ull * U * 4, hipMemcpyDeviceToHost, stream));
    }
    HIP_CHECK(hipStreamSynchronize(stream));
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventElapsedTime(&ms_final, S.ev[7], S.ev[8]));
    const uint32_t *any = counts.data(), *uniq = any + U, *assigned = uniq + U;
    uint64_t n_assigned = 0, n_any = 0, total_mass = 0, n_rows = 0;
    for (uint32_t i = 0; i < U; i++) {
        n_assigned += assigned[i];
        n_any += any[i];
        if (any[i]) {
            total_mass += mass[i];
            n_rows++;
        }
    }
    if (n_assigned != R || n_any != E)
        throw std::runtime_error("internal: " + std::to_string(R) + " reads of " + std::to_string(E) + " entries, " + std::to_string(n_assigned) + " assigned, " + std::to_string(n_any) + " counted at their TaxIDs");
    // ---- nothing can fail from here: the output fold takes the records, the caller the rows ----
    if (out) {
        out->commit(st, R);
        out->n_reads = n_reads;
        out->taxa.clear();
        for (uint32_t i = 0; i < U; i++)
            if (assigned[i]) out->taxa.push_back(taxa[i]);
    }
    if (rows) {
        rows->reserve(n_rows);
        for (uint32_t i = 0; i < U; i++)
            if (any[i]) rows->push_back(mtsv_abundance_row{taxa[i], 0, mass[i], any[i], uniq[i], assigned[i]});
    }
    if (info) *info = mtsv_abundance_info{R, E, n_rows, total_mass, iterations ? l1 : 0, iterations, converged};
    const float all_ms = ms_prepare[0] + ms_prepare[1] + ms_step + ms_delta + ms_final;
    if (device_ms) *device_ms = all_ms;
    if (trace)
        fprintf(stderr, "[abundance] %llu records, %llu reads, %llu entries over %u TaxIDs, %llu listed, %s adds, %u iterations (L1 %llu, tol %llu): %.3f ms\n",
                (unsigned long long)n, (unsigned long long)R, (unsigned long long)E, U, (unsigned long long)n_list, dense ? "LDS" : "global", iterations,
                (unsigned long long)l1, (unsigned long long)tol, all_ms);
    // MTSV_ABUND_TIMING=1: where a call spends its time (tools/abund_ab.py reads this line)
    if (S.timing)
        fprintf(stderr, "[abundance timing] records %llu reads %llu entries %llu taxa %u listed %llu dense %d blocks %u iterations %u; prepare %.3f ms, "
                        "step %.3f ms, delta %.3f ms, final %.3f ms, call %.3f ms\n",
                (unsigned long long)n, (unsigned long long)R, (unsigned long long)E, U, (unsigned long long)n_list, dense ? 1 : 0, blocks, iterations,
                ms_prepare[0] + ms_prepare[1], ms_step, ms_delta, ms_final, now_ms() - t0);
}

}  // namespace mtsv
