// host-side sanitizer run (ASan + UBSan) of the entry code of csrc/learn/ntuple_window.hip: every argument-refusal path of
// tpl_ntuple_window_prove, none of which reaches a HIP call; GPU code is not involved
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include "tpl_learn.h"

static std::string g_last;
namespace tpl_learn {
int fail_msg(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    g_last = buf;
    return code;
}
}

static int g_failed = 0;
static void refused(int rc, const char* word, const char* what) {
    if (rc != TPL_ERR_ARG || g_last.find(word) == std::string::npos || g_last.find("tpl_ntuple_window_prove:") != 0) {
        printf("NOT REFUSED as expected: %s (rc %d, message '%s')\n", what, rc, g_last.c_str());
        ++g_failed;
    }
    g_last.clear();
}
#define REFUSED(call, word) refused((call), word, #call)

// the entry with one argument list for the eight outputs: o = {solved, proved, solution_len, plan, bound, nodes, horizon, verdict}
struct Out {
    uint8_t* solved; uint8_t* proved; int32_t* solution_len; uint8_t* plan; int32_t* bound; uint32_t* nodes; uint8_t* horizon;
    uint8_t* verdict;
};
static int call(const void* a, const void* b, int64_t n, int32_t L, int32_t M, const int32_t* table, int64_t entries, float r_line,
                float r_win, float r_lose, float gamma, int32_t max_nodes, const uint8_t* skip, const Out& o) {
    return tpl_ntuple_window_prove(a, b, n, L, M, table, entries, r_line, r_win, r_lose, gamma, max_nodes, skip, o.solved, o.proved,
                                   o.solution_len, o.plan, o.bound, o.nodes, o.horizon, o.verdict, nullptr);
}

int main() {
    alignas(16) static unsigned char mem[256];
    // aligned, never dereferenced: every call below is refused before any HIP call
    const void* plane = mem;
    const int32_t* table = (const int32_t*)mem;
    const int32_t* odd_table = (const int32_t*)(mem + 2);
    const uint8_t* skip = mem + 1;                             // the mask has no alignment
    const Out ok{mem, mem, (int32_t*)mem, mem, (int32_t*)mem, (uint32_t*)mem, mem, mem};
    const Out none{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    const int64_t E = TPL_NTUPLE_ENTRIES_BUDGET;
    const float inf = std::numeric_limits<float>::infinity(), nan = std::nanf("");

    // the entry count: the four plain forms pass it (and are refused for the next thing), everything else is refused by it, first
    const int64_t plain[] = {TPL_NTUPLE_ENTRIES, TPL_NTUPLE_ENTRIES_3X3, TPL_NTUPLE_ENTRIES_FEAT, TPL_NTUPLE_ENTRIES_BUDGET};
    for (int64_t e : plain) REFUSED(call(nullptr, plane, 4, 2, 6, table, e, 1, 0, 0, 1, 100, nullptr, ok), "null");
    const int64_t other[] = {0, -1, 1, TPL_NTUPLE_ENTRIES_SUM, TPL_NTUPLE_ENTRIES_3X3_FEAT, TPL_NTUPLE_ENTRIES_STAGED, TPL_NTUPLE_ENTRIES_STAGED_3X3,
                             TPL_NTUPLE_ENTRIES_STAGED_SUM, TPL_NTUPLE_ENTRIES_BUDGET + 1, (int64_t)1 << 40};
    for (int64_t e : other) {
        REFUSED(call(plane, plane, 4, 2, 6, table, e, 1, 0, 0, 1, 100, nullptr, ok), "feat+spare");
        REFUSED(call(nullptr, nullptr, 0, 0, 0, nullptr, e, inf, nan, 0, inf, 0, nullptr, none), "entries must be");
    }

    // every pointer but skip and the stream is required
    REFUSED(call(nullptr, plane, 4, 2, 6, table, E, 1, 0, 0, 1, 100, nullptr, ok), "null");
    REFUSED(call(plane, nullptr, 4, 2, 6, table, E, 1, 0, 0, 1, 100, nullptr, ok), "null");
    REFUSED(call(plane, plane, 4, 2, 6, nullptr, E, 1, 0, 0, 1, 100, nullptr, ok), "null");
    for (int k = 0; k < 8; ++k) {
        Out o = ok;
        if (k == 0) o.solved = nullptr;
        if (k == 1) o.proved = nullptr;
        if (k == 2) o.solution_len = nullptr;
        if (k == 3) o.plan = nullptr;
        if (k == 4) o.bound = nullptr;
        if (k == 5) o.nodes = nullptr;
        if (k == 6) o.horizon = nullptr;
        if (k == 7) o.verdict = nullptr;
        REFUSED(call(plane, plane, 4, 2, 6, table, E, 1, 0, 0, 1, 100, skip, o), "null");
    }

    for (float bad : {inf, -inf, nan}) {
        REFUSED(call(plane, plane, 4, 2, 6, table, E, bad, 0, 0, 1, 100, nullptr, ok), "r_line, r_win and r_lose must be finite");
        REFUSED(call(plane, plane, 4, 2, 6, table, E, 1, bad, 0, 1, 100, nullptr, ok), "must be finite");
        REFUSED(call(plane, plane, 4, 2, 6, table, E, 1, 0, bad, 1, 100, nullptr, ok), "must be finite");
        REFUSED(call(plane, plane, 4, 2, 6, table, E, 1, 0, 0, bad, 100, nullptr, ok), "gamma must be finite");
    }

    REFUSED(call(plane, plane, 0, 2, 6, table, E, 1, 0, 0, 1, 100, nullptr, ok), "positive");
    REFUSED(call(plane, plane, -3, 2, 6, table, E, 1, 0, 0, 1, 100, nullptr, ok), "positive");
    REFUSED(call(plane, plane, (int64_t)1 << 31, 2, 6, table, E, 1, 0, 0, 1, 100, nullptr, ok), "2^31");
    REFUSED(call(plane, plane, (int64_t)1 << 40, 2, 6, table, E, 1, 0, 0, 1, 100, nullptr, ok), "2^31");
    REFUSED(call(plane, plane, 4, 0, 6, table, E, 1, 0, 0, 1, 100, nullptr, ok), "L and M");
    REFUSED(call(plane, plane, 4, 251, 6, table, E, 1, 0, 0, 1, 100, nullptr, ok), "L and M");
    REFUSED(call(plane, plane, 4, 2, 0, table, E, 1, 0, 0, 1, 100, nullptr, ok), "L and M");
    REFUSED(call(plane, plane, 4, 2, 255, table, E, 1, 0, 0, 1, 100, nullptr, ok), "L and M");
    REFUSED(call(plane, plane, 4, 2, 6, table, E, 1, 0, 0, 1, 0, nullptr, ok), "max_nodes must be in [1, 16777216]");
    REFUSED(call(plane, plane, 4, 2, 6, table, E, 1, 0, 0, 1, -1, nullptr, ok), "max_nodes");
    REFUSED(call(plane, plane, 4, 2, 6, table, E, 1, 0, 0, 1, (1 << 24) + 1, nullptr, ok), "max_nodes");
    REFUSED(call(mem + 8, plane, 4, 2, 6, table, E, 1, 0, 0, 1, 100, nullptr, ok), "planes must be 16-byte");
    REFUSED(call(plane, mem + 4, 4, 2, 6, table, E, 1, 0, 0, 1, 100, nullptr, ok), "planes must be 16-byte");
    REFUSED(call(plane, plane, 4, 2, 6, odd_table, E, 1, 0, 0, 1, 100, nullptr, ok), "table must be 4-byte");
    {
        Out o = ok; o.solution_len = (int32_t*)(mem + 2);
        REFUSED(call(plane, plane, 4, 2, 6, table, E, 1, 0, 0, 1, 100, nullptr, o), "solution_len must be 4-byte");
        o = ok; o.bound = (int32_t*)(mem + 2);
        REFUSED(call(plane, plane, 4, 2, 6, table, E, 1, 0, 0, 1, 100, nullptr, o), "bound must be 4-byte");
        o = ok; o.nodes = (uint32_t*)(mem + 2);
        REFUSED(call(plane, plane, 4, 2, 6, table, E, 1, 0, 0, 1, 100, nullptr, o), "nodes must be 4-byte");
    }
    // the largest arguments and an odd mask are not refused for themselves: a check that comes after them speaks
    REFUSED(call(plane, plane, ((int64_t)1 << 31) - 1, 250, 254, odd_table, E, 1, 0, 0, 1, 1 << 24, skip, ok), "table must be 4-byte");

    if (g_failed) { printf("%d refusal(s) missing\n", g_failed); return 1; }
    puts("sanitizer run ok");
    return 0;
}
