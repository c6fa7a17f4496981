// collapse_lines_check -- the host side of mtsv-collapse --on-gpu by itself (csrc/collapse_lines.hpp: files into lines, the
// dictionary of read IDs, the cut into layers and pieces, the staging of a piece), with no device and no library, so that
// it can run under the sanitizers:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/collapse_lines_check.cpp -o collapse_lines_check
//   ./collapse_lines_check PIECE_BYTES FILE...
// Every piece is staged into a heap block of exactly its size and checked: reads strictly ascending, one layer, the staged
// bytes are the lines' hit parts, the bytes within the bound unless the piece is a single line.  Prints one summary line and
// the lines put together again from the dictionary and the staged hits, ordered by (read, file, layer) -- the input of the
// fold, as text.  Exit 1 when a file has a line without a read ID, 2 when a check fails.
#include <cstdlib>
#include <map>
#include <memory>

#include "../mtsv_tools_amd/csrc/collapse_lines.hpp"

namespace mc = mtsv_collapse;

#define REQUIRE(c)                                                       \
    do {                                                                 \
        if (!(c)) {                                                      \
            fprintf(stderr, "check failed at line %d: %s\n", __LINE__, #c); \
            return 2;                                                    \
        }                                                                \
    } while (0)

int main(int argc, char** argv) {
    if (argc < 3) {
        fprintf(stderr, "usage: collapse_lines_check PIECE_BYTES FILE...\n");
        return 1;
    }
    const uint64_t piece_bytes = strtoull(argv[1], nullptr, 10);
    const size_t n_files = (size_t)argc - 2;
    std::vector<mc::FileBytes> bytes(n_files);
    std::vector<std::vector<mc::Line>> lines(n_files);
    for (size_t f = 0; f < n_files; f++) {
        if (!bytes[f].open(argv[f + 2])) {
            fprintf(stderr, "cannot read %s\n", argv[f + 2]);
            return 1;
        }
        std::string bad;
        if (!mc::split_lines(bytes[f].p, bytes[f].n, lines[f], &bad)) {
            fprintf(stderr, "InvalidHeader(%s)\n", bad.c_str());
            return 1;
        }
    }
    std::vector<const mc::Line*> dict;
    REQUIRE(mc::build_dictionary(lines, dict));
    for (size_t r = 1; r < dict.size(); r++) REQUIRE(std::string(dict[r - 1]->id, dict[r - 1]->id_len) < std::string(dict[r]->id, dict[r]->id_len));
    std::multimap<std::pair<uint32_t, std::pair<size_t, uint32_t>>, std::string> rebuilt;
    size_t n_lines = 0, n_pieces = 0;
    uint32_t max_layer = 0;
    std::vector<const mc::Line*> order;
    std::vector<mc::Piece> pieces;
    std::vector<uint64_t> line_off;
    std::vector<uint32_t> line_read;
    for (size_t f = 0; f < n_files; f++) {
        mc::cut_pieces(lines[f], piece_bytes, order, pieces);
        REQUIRE(order.size() == lines[f].size());
        size_t covered = 0;
        for (const auto& p : pieces) {
            REQUIRE(p.first == covered && p.last > p.first && p.last <= order.size());
            covered = p.last;
            REQUIRE(p.bytes <= piece_bytes || p.last - p.first == 1);
            std::unique_ptr<char[]> stage(new char[p.bytes]);  // (exactly the piece: one byte more is an error of the staging)
            mc::stage_piece(order, p, stage.get(), line_off, line_read);
            REQUIRE(line_off.size() == p.last - p.first + 1 && line_read.size() == p.last - p.first && line_off.back() == p.bytes);
            for (size_t i = p.first; i < p.last; i++) {
                const mc::Line& l = *order[i];
                const size_t k = i - p.first;
                REQUIRE(l.layer == order[p.first]->layer);
                REQUIRE(k == 0 || line_read[k - 1] < line_read[k]);
                REQUIRE(line_off[k + 1] - line_off[k] == l.hits_len);
                REQUIRE(l.read < dict.size() && mc::compare_ids(l, *dict[l.read]) == 0);
                REQUIRE(l.hits_len == 0 || memcmp(stage.get() + line_off[k], l.hits, l.hits_len) == 0);
                max_layer = std::max(max_layer, l.layer);
                rebuilt.emplace(std::make_pair(l.read, std::make_pair(f, l.layer)),
                                std::string(dict[l.read]->id, dict[l.read]->id_len) + ":" + std::string(stage.get() + line_off[k], l.hits_len));
            }
            n_pieces++;
        }
        REQUIRE(covered == order.size());
        n_lines += order.size();
    }
    printf("files %zu lines %zu ids %zu layers %u pieces %zu\n", n_files, n_lines, dict.size(), max_layer + 1, n_pieces);
    for (const auto& kv : rebuilt) printf("%s\n", kv.second.c_str());
    return 0;
}
