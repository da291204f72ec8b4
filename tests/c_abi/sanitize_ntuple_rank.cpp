// host-side sanitizer run (ASan + UBSan) of the entry code of csrc/learn/ntuple_rank.hip: every argument-refusal path of
// tpl_ntuple_rank, none of which reaches a HIP call; GPU code is not involved
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
    if (rc != TPL_ERR_ARG || g_last.find(word) == std::string::npos || g_last.find("tpl_ntuple_rank:") != 0) {
        printf("NOT REFUSED as expected: %s (rc %d, message '%s')\n", what, rc, g_last.c_str());
        ++g_failed;
    }
    g_last.clear();
}
#define REFUSED(call, word) refused((call), word, #call)

// the good call with one thing replaced at a time
struct Args {
    const void* a; const void* b; int64_t n; int32_t L, M; const int32_t* table; int64_t entries; const uint8_t* label;
    float r_line, r_win, r_lose, gamma, margin; int32_t prune;
    uint8_t *win, *loss, *greedy, *violated; float *gap, *err_win, *err_loss; void *win_a, *win_b, *loss_a, *loss_b;
};
static int call(const Args& x) {
    return tpl_ntuple_rank(x.a, x.b, x.n, x.L, x.M, x.table, x.entries, x.label, x.r_line, x.r_win, x.r_lose, x.gamma, x.margin, x.prune,
                           x.win, x.loss, x.greedy, x.violated, x.gap, x.err_win, x.err_loss, x.win_a, x.win_b, x.loss_a, x.loss_b, nullptr);
}

int main() {
    alignas(16) static unsigned char mem[256];
    // aligned, never dereferenced: every call below is refused before any HIP call
    float* f32 = (float*)mem;
    float* odd_f32 = (float*)(mem + 2);
    void* odd_plane = mem + 8;
    const float inf = std::numeric_limits<float>::infinity(), nan = std::nanf("");
    const Args ok{mem, mem, 4, 5, 10, (const int32_t*)mem, TPL_NTUPLE_ENTRIES_BUDGET, mem, 1, 10, -1, 0.99f, 0, 0,
                  mem, mem, mem, mem, f32, f32, f32, mem, mem, mem, mem};

    // the entry count: the four plain forms pass it (and are refused for the next thing), everything else is refused by it, first
    const int64_t plain[] = {TPL_NTUPLE_ENTRIES, TPL_NTUPLE_ENTRIES_3X3, TPL_NTUPLE_ENTRIES_FEAT, TPL_NTUPLE_ENTRIES_BUDGET};
    for (int64_t e : plain) { Args x = ok; x.entries = e; x.a = nullptr; REFUSED(call(x), "null"); }
    const int64_t other[] = {0, -1, 1, TPL_NTUPLE_ENTRIES_SUM, TPL_NTUPLE_ENTRIES_3X3_FEAT, TPL_NTUPLE_ENTRIES_STAGED, TPL_NTUPLE_ENTRIES_STAGED_3X3,
                             TPL_NTUPLE_ENTRIES_STAGED_SUM, TPL_NTUPLE_ENTRIES_BUDGET + 1, (int64_t)1 << 40};
    for (int64_t e : other) {
        Args x = ok; x.entries = e;
        REFUSED(call(x), "feat+spare");
        Args y{}; y.entries = e; y.prune = 7; y.margin = nan;
        REFUSED(call(y), "entries must be");
    }

    // the planes, n, L and M, the table
    { Args x = ok; x.a = nullptr; REFUSED(call(x), "null"); }
    { Args x = ok; x.b = nullptr; REFUSED(call(x), "null"); }
    { Args x = ok; x.n = 0; REFUSED(call(x), "positive"); }
    { Args x = ok; x.n = -3; REFUSED(call(x), "positive"); }
    { Args x = ok; x.n = ((int64_t)1 << 31) / 40 + 1; REFUSED(call(x), "40 n"); }
    { Args x = ok; x.n = (int64_t)1 << 40; REFUSED(call(x), "40 n"); }
    { Args x = ok; x.L = 0; REFUSED(call(x), "L and M"); }
    { Args x = ok; x.L = 251; REFUSED(call(x), "L and M"); }
    { Args x = ok; x.M = 0; REFUSED(call(x), "L and M"); }
    { Args x = ok; x.M = 255; REFUSED(call(x), "L and M"); }
    { Args x = ok; x.a = odd_plane; REFUSED(call(x), "planes must be 16-byte"); }
    { Args x = ok; x.b = odd_plane; REFUSED(call(x), "planes must be 16-byte"); }
    { Args x = ok; x.table = nullptr; REFUSED(call(x), "table is required"); }
    { Args x = ok; x.table = (const int32_t*)(mem + 4); REFUSED(call(x), "table must be 16-byte"); }

    // the label row and the eleven outputs
    { Args x = ok; x.label = nullptr; REFUSED(call(x), "label is required"); }
    { Args x = ok; x.win = nullptr; REFUSED(call(x), "every output"); }
    { Args x = ok; x.loss = nullptr; REFUSED(call(x), "every output"); }
    { Args x = ok; x.greedy = nullptr; REFUSED(call(x), "every output"); }
    { Args x = ok; x.violated = nullptr; REFUSED(call(x), "every output"); }
    { Args x = ok; x.gap = nullptr; REFUSED(call(x), "every output"); }
    { Args x = ok; x.err_win = nullptr; REFUSED(call(x), "every output"); }
    { Args x = ok; x.err_loss = nullptr; REFUSED(call(x), "every output"); }
    { Args x = ok; x.win_a = nullptr; REFUSED(call(x), "every output"); }
    { Args x = ok; x.win_b = nullptr; REFUSED(call(x), "every output"); }
    { Args x = ok; x.loss_a = nullptr; REFUSED(call(x), "every output"); }
    { Args x = ok; x.loss_b = nullptr; REFUSED(call(x), "every output"); }
    { Args x = ok; x.win_a = odd_plane; REFUSED(call(x), "must be 16-byte aligned"); }
    { Args x = ok; x.win_b = odd_plane; REFUSED(call(x), "must be 16-byte aligned"); }
    { Args x = ok; x.loss_a = odd_plane; REFUSED(call(x), "must be 16-byte aligned"); }
    { Args x = ok; x.loss_b = odd_plane; REFUSED(call(x), "must be 16-byte aligned"); }
    { Args x = ok; x.gap = odd_f32; REFUSED(call(x), "must be 4-byte aligned"); }
    { Args x = ok; x.err_win = odd_f32; REFUSED(call(x), "must be 4-byte aligned"); }
    { Args x = ok; x.err_loss = odd_f32; REFUSED(call(x), "must be 4-byte aligned"); }

    // the numbers
    for (float bad : {inf, -inf, nan}) {
        { Args x = ok; x.margin = bad; REFUSED(call(x), "margin must be finite"); }
        { Args x = ok; x.gamma = bad; REFUSED(call(x), "gamma must be finite"); }
        { Args x = ok; x.r_line = bad; REFUSED(call(x), "r_line, r_win and r_lose must be finite"); }
        { Args x = ok; x.r_win = bad; REFUSED(call(x), "must be finite"); }
        { Args x = ok; x.r_lose = bad; REFUSED(call(x), "must be finite"); }
    }

    // the prune: 0 or 1, and 1 under the budget form alone
    { Args x = ok; x.prune = 2; REFUSED(call(x), "prune must be 0 or 1"); }
    { Args x = ok; x.prune = -1; REFUSED(call(x), "prune must be 0 or 1"); }
    for (int64_t e : {(int64_t)TPL_NTUPLE_ENTRIES, (int64_t)TPL_NTUPLE_ENTRIES_3X3, (int64_t)TPL_NTUPLE_ENTRIES_FEAT}) {
        Args x = ok; x.entries = e; x.prune = 1;
        REFUSED(call(x), "budget table");
    }
    // the largest game is not refused for its size: a check that comes after it speaks; and prune = 1 passes under the budget form
    { Args x = ok; x.L = 250; x.M = 254; x.n = ((int64_t)1 << 31) / 40; x.prune = 1; x.gap = odd_f32; REFUSED(call(x), "must be 4-byte aligned"); }

    if (g_failed) { printf("%d refusal(s) missing\n", g_failed); return 1; }
    puts("sanitizer run ok");
    return 0;
}
