// taxonomy.cpp -- NCBI nodes.dmp into mtsv::Taxonomy (taxonomy.hpp).  Host only.
#include "taxonomy.hpp"

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstring>
#include <stdexcept>

namespace mtsv {

namespace {

struct RawNode {
    uint32_t id, parent;
    uint32_t rank;  // index into the ranks as they were met, then the rank code
    uint64_t line;
};

bool is_blank(char c) { return c == ' ' || c == '\t' || c == '\r'; }

// [b, e) without the blanks and tabs around it
void trim(const char*& b, const char*& e) {
    while (b < e && is_blank(*b)) b++;
    while (e > b && is_blank(e[-1])) e--;
}

// 1 to 10 decimal digits with a value up to 4294967295
bool parse_id(const char* b, const char* e, uint32_t* out) {
    if (b == e || e - b > 10) return false;
    uint64_t v = 0;
    for (const char* p = b; p < e; p++) {
        if (*p < '0' || *p > '9') return false;
        v = v * 10 + (uint64_t)(*p - '0');
    }
    if (v > 0xffffffffull) return false;
    *out = (uint32_t)v;
    return true;
}

std::string read_file(const std::string& path) {
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) throw std::runtime_error("io: cannot open " + path);
    std::string s;
    char buf[1 << 16];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) s.append(buf, got);
    const bool bad = ferror(f) != 0;
    fclose(f);
    if (bad) throw std::runtime_error("io: short read on " + path);
    return s;
}

std::atomic<uint64_t> g_serial{0};

}  // namespace

Taxonomy Taxonomy::load(const std::string& path) {
    const std::string text = read_file(path);
    std::vector<RawNode> nodes;
    std::vector<std::string> met;  // rank strings in the order they were met (a handful: searched linearly)
    uint64_t line_no = 0;
    for (size_t at = 0; at < text.size();) {
        const char* nl = (const char*)memchr(text.data() + at, '\n', text.size() - at);
        const char *b = text.data() + at, *e = nl ? nl : text.data() + text.size();
        at = (size_t)(e - text.data()) + 1;
        line_no++;
        const char *lb = b, *le = e;
        trim(lb, le);
        if (lb == le) continue;
        const char *fb[3], *fe[3];
        int nf = 0;
        for (const char* p = b; nf < 3;) {
            const char* bar = (const char*)memchr(p, '|', (size_t)(e - p));
            fb[nf] = p;
            fe[nf] = bar ? bar : e;
            trim(fb[nf], fe[nf]);
            nf++;
            if (!bar) break;
            p = bar + 1;
        }
        const std::string where = "format: " + path + ": line " + std::to_string(line_no) + ": ";
        if (nf < 3) throw std::runtime_error(where + "fewer than three fields (TaxID | parent TaxID | rank)");
        RawNode n{0, 0, 0, line_no};
        if (!parse_id(fb[0], fe[0], &n.id)) throw std::runtime_error(where + "the TaxID is not 1 to 10 digits with a value up to 4294967295");
        if (!parse_id(fb[1], fe[1], &n.parent)) throw std::runtime_error(where + "the parent TaxID is not 1 to 10 digits with a value up to 4294967295");
        if (n.id == 0 || n.parent == 0) throw std::runtime_error(where + "TaxID 0 (it is the super-root's)");
        const std::string rank(fb[2], fe[2]);
        size_t k = 0;
        while (k < met.size() && met[k] != rank) k++;
        if (k == met.size()) met.push_back(rank);
        n.rank = (uint32_t)k;
        nodes.push_back(n);
    }
    std::stable_sort(nodes.begin(), nodes.end(), [](const RawNode& a, const RawNode& b) { return a.id < b.id; });
    for (size_t k = 1; k < nodes.size(); k++)
        if (nodes[k].id == nodes[k - 1].id)
            throw std::runtime_error("format: " + path + ": line " + std::to_string(nodes[k].line) + ": TaxID " + std::to_string(nodes[k].id) +
                                     " is listed twice (first on line " + std::to_string(nodes[k - 1].line) + ")");
    Taxonomy t;
    // ---- rank codes: the place of the string among the distinct strings, ascending by bytes ----
    t.rank_names = met;
    std::sort(t.rank_names.begin(), t.rank_names.end());
    std::vector<uint32_t> code(met.size());
    for (size_t k = 0; k < met.size(); k++) code[k] = (uint32_t)(std::lower_bound(t.rank_names.begin(), t.rank_names.end(), met[k]) - t.rank_names.begin());
    const size_t n = nodes.size();
    t.ids.resize(n);
    t.parents.resize(n);
    t.ranks.resize(n);
    for (size_t k = 0; k < n; k++) {
        t.ids[k] = nodes[k].id;
        t.parents[k] = nodes[k].parent;
        t.ranks[k] = code[nodes[k].rank];
    }
    // ---- the parents' places; those without a line are the implied roots ----
    constexpr uint32_t kNone = 0xffffffffu;
    std::vector<uint32_t> up(n);  // the place of the parent's line; kNone for roots and children of implied roots
    for (size_t k = 0; k < n; k++) {
        up[k] = kNone;
        if (t.parents[k] == t.ids[k]) continue;
        const auto it = std::lower_bound(t.ids.begin(), t.ids.end(), t.parents[k]);
        if (it != t.ids.end() && *it == t.parents[k]) up[k] = (uint32_t)(it - t.ids.begin());
        else t.implied.push_back(t.parents[k]);
    }
    std::sort(t.implied.begin(), t.implied.end());
    t.implied.erase(std::unique(t.implied.begin(), t.implied.end()), t.implied.end());
    // ---- depths, and with them the cycles: a walk up from every node whose depth is not known, marking its path ----
    std::vector<uint32_t> depth(n, 0);  // 0: not known; kNone: on the path of the walk under way
    std::vector<uint32_t> path_up;
    t.max_depth = t.implied.empty() ? 0 : 1;
    for (size_t s = 0; s < n; s++) {
        if (depth[s]) continue;
        path_up.clear();
        uint32_t k = (uint32_t)s, base = 0;
        for (;;) {
            if (depth[k] == kNone)
                throw std::runtime_error("format: " + path + ": line " + std::to_string(nodes[k].line) + ": TaxID " + std::to_string(t.ids[k]) +
                                         " is its own ancestor (a cycle other than a root's self-parent)");
            if (depth[k]) {
                base = depth[k];
                break;
            }
            depth[k] = kNone;
            path_up.push_back(k);
            if (up[k] == kNone) {  // a root (the super-root above it), or the child of an implied root
                base = t.parents[k] == t.ids[k] ? 0 : 1;
                break;
            }
            k = up[k];
        }
        for (size_t j = path_up.size(); j-- > 0;) depth[path_up[j]] = ++base;
        t.max_depth = std::max(t.max_depth, depth[s]);
    }
    t.serial = ++g_serial;
    return t;
}

bool Taxonomy::lookup(uint32_t tax_id, uint32_t* parent, uint32_t* rank) const {
    *parent = 0;
    *rank = kRankUnknown;
    if (tax_id == 0) return true;
    const auto it = std::lower_bound(ids.begin(), ids.end(), tax_id);
    if (it != ids.end() && *it == tax_id) {
        const size_t k = (size_t)(it - ids.begin());
        *parent = parents[k] == tax_id ? 0 : parents[k];
        *rank = ranks[k];
        return true;
    }
    return std::binary_search(implied.begin(), implied.end(), tax_id);
}

}  // namespace mtsv
