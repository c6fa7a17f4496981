// cli_common.hpp -- what the command lines share: the reference's log lines and panics, list splitting, a clock and
// "write all of it".  Header only; nothing of HIP or libmtsv_amd, so mtsv-partition's plain g++ build takes it too.
#pragma once
#include <unistd.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <string>
#include <vector>

namespace mtsv_cli {

inline bool& verbose() {  // -v: DEBUG lines are printed
    static bool v = false;
    return v;
}

// util.rs:10-24: "[LEVEL ts tool] msg" on stdout
inline void logmsg(const char* tool, const char* level, const std::string& msg) {
    if (!verbose() && !strcmp(level, "DEBUG")) return;
    char ts[32];
    time_t t = time(nullptr);
    strftime(ts, sizeof ts, "%Y-%m-%d %H:%M:%S", localtime(&t));
    printf("[%s %s %s] %s\n", level, ts, tool, msg.c_str());
    fflush(stdout);
}

[[noreturn]] inline void panic(const std::string& msg) {  // the reference's expect()/panic!() paths
    fprintf(stderr, "thread 'main' panicked: %s\n", msg.c_str());
    exit(101);
}

// the tokens of "a,b,..": every one, empty ones too ("" is one empty token), or only those that hold something
inline std::vector<std::string> split_list(const std::string& s, char sep, bool keep_empty = false) {
    std::vector<std::string> out;
    for (size_t at = 0; at <= s.size();) {
        size_t c = s.find(sep, at);
        if (c == std::string::npos) c = s.size();
        if (keep_empty || c > at) out.push_back(s.substr(at, c - at));
        at = c + 1;
    }
    return out;
}

inline double now_s() {  // monotonic seconds
    struct timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return t.tv_sec + t.tv_nsec * 1e-9;
}

inline bool write_all(int fd, const char* q, uint64_t len) {
    for (uint64_t done = 0; done < len;) {
        const ssize_t r = ::write(fd, q + done, len - done);
        if (r <= 0) return false;
        done += (uint64_t)r;
    }
    return true;
}
inline bool pwrite_all(int fd, const char* q, uint64_t len, off_t at) {
    for (uint64_t done = 0; done < len;) {
        const ssize_t r = ::pwrite(fd, q + done, len - done, at + (off_t)done);
        if (r <= 0) return false;
        done += (uint64_t)r;
    }
    return true;
}

// MTSV_CLI_MARKS=1: the set-up phases on stderr as they end, in ms since the first call (the first thing main does)
inline void setup_mark(const char* what) {
    static const bool on = getenv("MTSV_CLI_MARKS") != nullptr;
    static const double t0 = now_s();
    if (on) fprintf(stderr, "[cli set-up] %9.3f ms  %s\n", (now_s() - t0) * 1e3, what);
}

}  // namespace mtsv_cli
