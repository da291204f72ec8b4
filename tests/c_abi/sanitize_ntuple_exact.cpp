// host-side sanitizer run (ASan + UBSan) of the entry code of csrc/learn/ntuple_exact.hip: every argument-refusal path of
// tpl_ntuple_exact, none of which reaches a HIP call; GPU code is not involved
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
    if (rc != TPL_ERR_ARG || g_last.find(word) == std::string::npos || g_last.find("tpl_ntuple_exact:") != 0) {
        printf("NOT REFUSED as expected: %s (rc %d, message '%s')\n", what, rc, g_last.c_str());
        ++g_failed;
    }
    g_last.clear();
}
#define REFUSED(call, word) refused((call), word, #call)

int main() {
    alignas(16) static unsigned char mem[256];
    // aligned, never dereferenced: every call below is refused before any HIP call
    const int16_t* rows = (const int16_t*)mem;
    const uint8_t* pieces = mem;
    const int32_t* table = (const int32_t*)mem;
    uint8_t* u8 = mem;
    int32_t* i32 = (int32_t*)mem;
    uint32_t* u32 = (uint32_t*)mem;
    const int16_t* odd_rows = (const int16_t*)(mem + 1);
    const int32_t* odd_table = (const int32_t*)(mem + 2);
    int32_t* odd_i32 = (int32_t*)(mem + 2);
    uint32_t* odd_u32 = (uint32_t*)(mem + 2);
    const int64_t E = TPL_NTUPLE_ENTRIES_BUDGET;
    const float inf = std::numeric_limits<float>::infinity(), nan = std::nanf("");

    // the entry count: the four plain forms pass it (and are refused for the next thing), everything else is refused by it
    const int64_t plain[] = {TPL_NTUPLE_ENTRIES, TPL_NTUPLE_ENTRIES_3X3, TPL_NTUPLE_ENTRIES_FEAT, TPL_NTUPLE_ENTRIES_BUDGET};
    for (int64_t e : plain) REFUSED(tpl_ntuple_exact(nullptr, pieces, 4, 2, 6, table, e, 1, 0, 0, 1, 100, 1, u8, u8, i32, u8, i32, u32, nullptr), "null");
    const int64_t other[] = {0, -1, 1, TPL_NTUPLE_ENTRIES_SUM, TPL_NTUPLE_ENTRIES_3X3_FEAT, TPL_NTUPLE_ENTRIES_STAGED, TPL_NTUPLE_ENTRIES_STAGED_3X3,
                             TPL_NTUPLE_ENTRIES_STAGED_SUM, TPL_NTUPLE_ENTRIES_BUDGET + 1, (int64_t)1 << 40};
    for (int64_t e : other) {
        REFUSED(tpl_ntuple_exact(rows, pieces, 4, 2, 6, table, e, 1, 0, 0, 1, 100, 1, u8, u8, i32, u8, i32, u32, nullptr), "feat+spare");
        REFUSED(tpl_ntuple_exact(nullptr, nullptr, 0, 0, 0, nullptr, e, 1, 0, 0, 1, 0, 7, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), "entries must be");
    }

    REFUSED(tpl_ntuple_exact(nullptr, pieces, 4, 2, 6, table, E, 1, 0, 0, 1, 100, 1, u8, u8, i32, u8, i32, u32, nullptr), "null");
    REFUSED(tpl_ntuple_exact(rows, nullptr, 4, 2, 6, table, E, 1, 0, 0, 1, 100, 1, u8, u8, i32, u8, i32, u32, nullptr), "null");
    REFUSED(tpl_ntuple_exact(rows, pieces, 4, 2, 6, nullptr, E, 1, 0, 0, 1, 100, 1, u8, u8, i32, u8, i32, u32, nullptr), "null");
    REFUSED(tpl_ntuple_exact(rows, pieces, 4, 2, 6, table, E, 1, 0, 0, 1, 100, 1, nullptr, u8, i32, u8, i32, u32, nullptr), "null");
    REFUSED(tpl_ntuple_exact(rows, pieces, 4, 2, 6, table, E, 1, 0, 0, 1, 100, 1, u8, nullptr, i32, u8, i32, u32, nullptr), "null");
    REFUSED(tpl_ntuple_exact(rows, pieces, 4, 2, 6, table, E, 1, 0, 0, 1, 100, 1, u8, u8, nullptr, u8, i32, u32, nullptr), "null");
    REFUSED(tpl_ntuple_exact(rows, pieces, 4, 2, 6, table, E, 1, 0, 0, 1, 100, 1, u8, u8, i32, nullptr, i32, u32, nullptr), "null");
    REFUSED(tpl_ntuple_exact(rows, pieces, 4, 2, 6, table, E, 1, 0, 0, 1, 100, 1, u8, u8, i32, u8, nullptr, u32, nullptr), "null");
    REFUSED(tpl_ntuple_exact(rows, pieces, 4, 2, 6, table, E, 1, 0, 0, 1, 100, 1, u8, u8, i32, u8, i32, nullptr, nullptr), "null");

    for (float bad : {inf, -inf, nan}) {
        REFUSED(tpl_ntuple_exact(rows, pieces, 4, 2, 6, table, E, bad, 0, 0, 1, 100, 1, u8, u8, i32, u8, i32, u32, nullptr), "must be finite");
        REFUSED(tpl_ntuple_exact(rows, pieces, 4, 2, 6, table, E, 1, bad, 0, 1, 100, 1, u8, u8, i32, u8, i32, u32, nullptr), "must be finite");
        REFUSED(tpl_ntuple_exact(rows, pieces, 4, 2, 6, table, E, 1, 0, bad, 1, 100, 1, u8, u8, i32, u8, i32, u32, nullptr), "must be finite");
        REFUSED(tpl_ntuple_exact(rows, pieces, 4, 2, 6, table, E, 1, 0, 0, bad, 100, 1, u8, u8, i32, u8, i32, u32, nullptr), "gamma must be finite");
    }

    REFUSED(tpl_ntuple_exact(rows, pieces, 0, 2, 6, table, E, 1, 0, 0, 1, 100, 1, u8, u8, i32, u8, i32, u32, nullptr), "positive");
    REFUSED(tpl_ntuple_exact(rows, pieces, -3, 2, 6, table, E, 1, 0, 0, 1, 100, 1, u8, u8, i32, u8, i32, u32, nullptr), "positive");
    REFUSED(tpl_ntuple_exact(rows, pieces, (int64_t)1 << 31, 2, 6, table, E, 1, 0, 0, 1, 100, 1, u8, u8, i32, u8, i32, u32, nullptr), "2^31");
    REFUSED(tpl_ntuple_exact(rows, pieces, (int64_t)1 << 40, 2, 6, table, E, 1, 0, 0, 1, 100, 1, u8, u8, i32, u8, i32, u32, nullptr), "2^31");
    REFUSED(tpl_ntuple_exact(rows, pieces, 4, 0, 6, table, E, 1, 0, 0, 1, 100, 1, u8, u8, i32, u8, i32, u32, nullptr), "L and M");
    REFUSED(tpl_ntuple_exact(rows, pieces, 4, 251, 6, table, E, 1, 0, 0, 1, 100, 1, u8, u8, i32, u8, i32, u32, nullptr), "L and M");
    REFUSED(tpl_ntuple_exact(rows, pieces, 4, 2, 0, table, E, 1, 0, 0, 1, 100, 1, u8, u8, i32, u8, i32, u32, nullptr), "L and M");
    REFUSED(tpl_ntuple_exact(rows, pieces, 4, 2, 255, table, E, 1, 0, 0, 1, 100, 1, u8, u8, i32, u8, i32, u32, nullptr), "L and M");
    REFUSED(tpl_ntuple_exact(rows, pieces, 4, 2, 6, table, E, 1, 0, 0, 1, 0, 1, u8, u8, i32, u8, i32, u32, nullptr), "max_nodes must be in [1, 16777216]");
    REFUSED(tpl_ntuple_exact(rows, pieces, 4, 2, 6, table, E, 1, 0, 0, 1, -1, 1, u8, u8, i32, u8, i32, u32, nullptr), "max_nodes");
    REFUSED(tpl_ntuple_exact(rows, pieces, 4, 2, 6, table, E, 1, 0, 0, 1, (1 << 24) + 1, 1, u8, u8, i32, u8, i32, u32, nullptr), "max_nodes");
    REFUSED(tpl_ntuple_exact(rows, pieces, 4, 2, 6, table, E, 1, 0, 0, 1, 100, 2, u8, u8, i32, u8, i32, u32, nullptr), "shortest must be 0 or 1");
    REFUSED(tpl_ntuple_exact(rows, pieces, 4, 2, 6, table, E, 1, 0, 0, 1, 100, -1, u8, u8, i32, u8, i32, u32, nullptr), "shortest must be 0 or 1");
    REFUSED(tpl_ntuple_exact(odd_rows, pieces, 4, 2, 6, table, E, 1, 0, 0, 1, 100, 1, u8, u8, i32, u8, i32, u32, nullptr), "rows must be 2-byte");
    REFUSED(tpl_ntuple_exact(rows, pieces, 4, 2, 6, odd_table, E, 1, 0, 0, 1, 100, 1, u8, u8, i32, u8, i32, u32, nullptr), "table must be 4-byte");
    REFUSED(tpl_ntuple_exact(rows, pieces, 4, 2, 6, table, E, 1, 0, 0, 1, 100, 1, u8, u8, odd_i32, u8, i32, u32, nullptr), "solution_len must be 4-byte");
    REFUSED(tpl_ntuple_exact(rows, pieces, 4, 2, 6, table, E, 1, 0, 0, 1, 100, 1, u8, u8, i32, u8, odd_i32, u32, nullptr), "bound must be 4-byte");
    REFUSED(tpl_ntuple_exact(rows, pieces, 4, 2, 6, table, E, 1, 0, 0, 1, 100, 1, u8, u8, i32, u8, i32, odd_u32, nullptr), "nodes must be 4-byte");
    // the largest game and the largest node budget are not refused for their size: a check that comes after them speaks
    REFUSED(tpl_ntuple_exact(odd_rows, pieces, 4, 250, 254, table, E, 1, 0, 0, 1, 1 << 24, 0, u8, u8, i32, u8, i32, u32, nullptr), "rows must be 2-byte");

    if (g_failed) { printf("%d refusal(s) missing\n", g_failed); return 1; }
    puts("sanitizer run ok");
    return 0;
}
