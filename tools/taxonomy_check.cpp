// taxonomy_check -- the taxonomy loader by itself (csrc/taxonomy.cpp: nodes.dmp into a tree, its refusals, the lookups), with
// no device and nothing else of the library, so that it can run under the sanitizers:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/taxonomy_check.cpp mtsv_tools_amd/csrc/taxonomy.cpp -o taxonomy_check
//   ./taxonomy_check FILE...
// Every file is loaded; one that loads is walked: every listed node and implied root is looked up, its chain of parents
// followed to the super-root -- within max_depth steps, the deepest chain exactly max_depth long --, its rank name read, and
// TaxIDs next to the listed ones are looked up as unknown.  Prints one line per file: its counts, or the refusal.  Exit 0 when
// every file loaded or was refused with a format or io message, 2 when a check fails.
#include <cstdio>
#include <cstring>
#include <stdexcept>

#include "../mtsv_tools_amd/csrc/taxonomy.hpp"

#define REQUIRE(c)                                                       \
    do {                                                                 \
        if (!(c)) {                                                      \
            fprintf(stderr, "check failed at line %d: %s\n", __LINE__, #c); \
            return 2;                                                    \
        }                                                                \
    } while (0)

int main(int argc, char** argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: taxonomy_check FILE...\n");
        return 1;
    }
    for (int f = 1; f < argc; f++) {
        mtsv::Taxonomy t;
        try {
            t = mtsv::Taxonomy::load(argv[f]);
        } catch (const std::runtime_error& e) {
            REQUIRE(strncmp(e.what(), "format: ", 8) == 0 || strncmp(e.what(), "io: ", 4) == 0);
            printf("%s: refused: %s\n", argv[f], e.what());
            continue;
        }
        REQUIRE(t.ids.size() == t.parents.size() && t.ids.size() == t.ranks.size() && t.serial != 0);
        for (size_t k = 1; k < t.ids.size(); k++) REQUIRE(t.ids[k - 1] < t.ids[k]);
        for (size_t k = 1; k < t.rank_names.size(); k++) REQUIRE(t.rank_names[k - 1] < t.rank_names[k]);
        uint32_t deepest = 0, p = 0, r = 0;
        size_t n_roots = 0;
        std::vector<uint32_t> all = t.ids;
        all.insert(all.end(), t.implied.begin(), t.implied.end());
        for (uint32_t id : all) {
            REQUIRE(id != 0 && t.lookup(id, &p, &r));
            REQUIRE(r == mtsv::kRankUnknown || r < t.rank_names.size());
            REQUIRE(strlen(t.rank_name(r)) < 1u << 20);
            n_roots += p == 0;
            uint32_t depth = 1, a = id;
            while (true) {
                REQUIRE(t.lookup(a, &p, &r));
                if (!p) break;
                a = p;
                REQUIRE(++depth <= t.max_depth);
            }
            deepest = depth > deepest ? depth : deepest;
            for (uint32_t near : {id - 1, id + 1}) {  // (wraps at both ends of the range: still a lookup like any other)
                const bool known = t.lookup(near, &p, &r);
                REQUIRE(known || (p == 0 && r == mtsv::kRankUnknown));
            }
        }
        REQUIRE(deepest == t.max_depth);
        REQUIRE(t.lookup(0, &p, &r) && p == 0 && r == mtsv::kRankUnknown);
        REQUIRE(strcmp(t.rank_name(mtsv::kRankUnknown), "-") == 0);
        printf("%s: nodes %zu implied_roots %zu roots %zu ranks %zu max_depth %u\n", argv[f], t.ids.size(), t.implied.size(), n_roots, t.rank_names.size(),
               t.max_depth);
    }
    return 0;
}
