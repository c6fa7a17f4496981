// collapse_lines.hpp -- the host side of mtsv-collapse --on-gpu that needs no device: result files read into memory and cut
// into lines, the dictionary that numbers the read IDs, and the cut of a file into the pieces mtsv_fold_add_text takes.
// Header only and free of the library, so that it can be run by itself (tools/collapse_lines_check.cpp).
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

namespace mtsv_collapse {

// a whole file: mapped, or read when it cannot be mapped (a pipe, a file system without mmap)
struct FileBytes {
    const char* p = nullptr;
    size_t n = 0;
    void* mapped = nullptr;
    std::vector<char> owned;
    FileBytes() = default;
    FileBytes(const FileBytes&) = delete;
    FileBytes& operator=(const FileBytes&) = delete;
    FileBytes(FileBytes&& o) noexcept { *this = std::move(o); }
    FileBytes& operator=(FileBytes&& o) noexcept {
        release();
        n = o.n;
        mapped = o.mapped;
        owned = std::move(o.owned);
        p = mapped ? (const char*)mapped : owned.data();
        o.p = nullptr;
        o.n = 0;
        o.mapped = nullptr;
        return *this;
    }
    ~FileBytes() { release(); }
    void release() {
        if (mapped) munmap(mapped, n);
        mapped = nullptr;
        p = nullptr;
        n = 0;
    }
    bool open(const std::string& path) {
        release();
        owned.clear();
        const int fd = ::open(path.c_str(), O_RDONLY);
        if (fd < 0) return false;
        struct stat st;
        if (fstat(fd, &st) == 0 && S_ISREG(st.st_mode) && st.st_size > 0) {
            void* m = mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
            if (m != MAP_FAILED) {
                mapped = m;
                p = (const char*)m;
                n = (size_t)st.st_size;
                close(fd);
                return true;
            }
        }
        char buf[1 << 16];
        for (;;) {
            const ssize_t k = read(fd, buf, sizeof buf);
            if (k < 0) {
                close(fd);
                return false;
            }
            if (k == 0) break;
            owned.insert(owned.end(), buf, buf + k);
        }
        close(fd);
        p = owned.data();
        n = owned.size();
        return true;
    }
};

struct Line {
    const char* id;
    const char* hits;
    uint64_t id_len, hits_len;
    uint32_t read;   // the rank of the ID in the dictionary
    uint32_t layer;  // how many earlier lines of its file name the same ID
};

// The lines of a file by mtsv-collapse's rules: cut at '\n', trailing '\r' and '\n' trimmed, lines of blanks and tabs skipped,
// the ID is what stands before the last ':' and must not be empty.  False, with the offending line in *bad, for a line
// without ':' or with an empty ID.
inline bool split_lines(const char* data, size_t n, std::vector<Line>& out, std::string* bad) {
    size_t at = 0;
    while (at < n) {
        const char* nl = (const char*)memchr(data + at, '\n', n - at);
        const size_t end = nl ? (size_t)(nl - data) : n;
        size_t e = end;
        while (e > at && data[e - 1] == '\r') e--;
        size_t b = at;
        while (b < e && (data[b] == ' ' || data[b] == '\t')) b++;
        if (b < e) {  // (not blank)
            size_t c = e;
            while (c > at && data[c - 1] != ':') c--;
            if (c <= at + 1) {  // (no ':' at all, or the last one is the line's first byte)
                if (bad) bad->assign(data + at, e - at);
                return false;
            }
            out.push_back(Line{data + at, data + c, (uint64_t)(c - 1 - at), (uint64_t)(e - c), 0, 0});
        }
        at = end + 1;
    }
    return true;
}

// std::string's order: bytes as unsigned, the shorter of two that agree first
inline int compare_ids(const Line& a, const Line& b) {
    const int c = memcmp(a.id, b.id, (size_t)std::min(a.id_len, b.id_len));
    if (c) return c;
    return a.id_len < b.id_len ? -1 : a.id_len > b.id_len ? 1 : 0;
}

// The dictionary over the lines of all files: the distinct IDs in std::string order; every line's `read` becomes its ID's
// rank.  dict[r]: a line that carries ID r.  False when there are 2^32 distinct IDs or more.
inline bool build_dictionary(std::vector<std::vector<Line>>& files, std::vector<const Line*>& dict) {
    std::vector<Line*> all;
    for (auto& f : files)
        for (auto& l : f) all.push_back(&l);
    std::sort(all.begin(), all.end(), [](const Line* a, const Line* b) { return compare_ids(*a, *b) < 0; });
    dict.clear();
    for (size_t i = 0; i < all.size(); i++) {
        if (i == 0 || compare_ids(*all[i - 1], *all[i]) != 0) {
            if (dict.size() >= 0xffffffffull) return false;
            dict.push_back(all[i]);
        }
        all[i]->read = (uint32_t)(dict.size() - 1);
    }
    return true;
}

// One call of mtsv_fold_add_text: lines order[first .. last) of a file
struct Piece {
    size_t first, last;
    uint64_t bytes;
};

// A file's lines in the order of the calls, and the calls.  The k-th line that names an ID goes to layer k; the order is by
// (layer, read), so that every layer -- and every piece, which is a stretch of one layer -- has strictly ascending reads.  A
// piece ends before the line that would take its hit bytes above piece_bytes; a line longer than that is a piece by itself.
inline void cut_pieces(std::vector<Line>& lines, uint64_t piece_bytes, std::vector<const Line*>& order, std::vector<Piece>& pieces) {
    std::vector<Line*> by_read;
    for (auto& l : lines) by_read.push_back(&l);
    std::stable_sort(by_read.begin(), by_read.end(), [](const Line* a, const Line* b) { return a->read < b->read; });
    for (size_t i = 0; i < by_read.size(); i++) by_read[i]->layer = i && by_read[i - 1]->read == by_read[i]->read ? by_read[i - 1]->layer + 1 : 0;
    std::stable_sort(by_read.begin(), by_read.end(), [](const Line* a, const Line* b) { return a->layer < b->layer; });
    order.assign(by_read.begin(), by_read.end());
    pieces.clear();
    for (size_t i = 0; i < order.size();) {
        Piece p{i, i, 0};
        while (p.last < order.size() && order[p.last]->layer == order[i]->layer && (p.last == i || p.bytes + order[p.last]->hits_len <= piece_bytes)) {
            p.bytes += order[p.last]->hits_len;
            p.last++;
        }
        pieces.push_back(p);
        i = p.last;
    }
}

// The arrays of one call: the hit parts of the piece's lines end to end in dst (p.bytes of room), their offsets and reads
inline void stage_piece(const std::vector<const Line*>& order, const Piece& p, char* dst, std::vector<uint64_t>& line_off, std::vector<uint32_t>& line_read) {
    line_off.assign(1, 0);
    line_read.clear();
    uint64_t at = 0;
    for (size_t i = p.first; i < p.last; i++) {
        if (order[i]->hits_len) memcpy(dst + at, order[i]->hits, (size_t)order[i]->hits_len);
        at += order[i]->hits_len;
        line_off.push_back(at);
        line_read.push_back(order[i]->read);
    }
}

}  // namespace mtsv_collapse
