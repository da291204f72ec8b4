// host-side sanitizer run (ASan + UBSan) of the entry code of csrc/learn/curriculum.hip: every argument-refusal path of
// tpl_config_index, tpl_pool_tally and tpl_pool_resample, none of which reaches a HIP call; GPU code is not involved
#include <cstdarg>
#include <cstdio>
#include <cstring>
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
    if (rc != TPL_ERR_ARG || g_last.find(word) == std::string::npos) {
        printf("NOT REFUSED as expected: %s (rc %d, message '%s')\n", what, rc, g_last.c_str());
        ++g_failed;
    }
    g_last.clear();
}
#define REFUSED(call, word) refused((call), word, #call)

int main() {
    alignas(16) static unsigned char mem[256];
    void* p = mem;                 // aligned, never dereferenced: every call below is refused before any HIP call
    void* odd = mem + 1;
    void* four = mem + 4;
    uint32_t* idx = (uint32_t*)mem;
    uint8_t* slot = mem;
    int32_t* t = (int32_t*)mem;
    const int64_t big = (int64_t)1 << 32;

    REFUSED(tpl_config_index(nullptr, p, p, 4, 0, 0, 0, 7, 0, idx, slot, nullptr), "null");
    REFUSED(tpl_config_index(p, nullptr, p, 4, 0, 0, 0, 7, 0, idx, slot, nullptr), "null");
    REFUSED(tpl_config_index(p, p, nullptr, 4, 0, 0, 0, 7, 0, idx, slot, nullptr), "null");
    REFUSED(tpl_config_index(p, p, p, 0, 0, 0, 0, 7, 0, idx, slot, nullptr), "n must");
    REFUSED(tpl_config_index(p, p, p, (int64_t)1 << 31, 0, 0, 0, 7, 0, idx, slot, nullptr), "n must");
    REFUSED(tpl_config_index(four, p, p, 4, 0, 0, 0, 7, 0, idx, slot, nullptr), "16-byte");
    REFUSED(tpl_config_index(p, p, four, 4, 0, 0, 0, 7, 0, idx, slot, nullptr), "8-byte");
    REFUSED(tpl_config_index(p, p, p, 4, -1, 0, 0, 7, 0, idx, slot, nullptr), "global_offset");
    REFUSED(tpl_config_index(p, p, p, 4, 0, 0, 2, 7, 0, idx, slot, nullptr), "assign_mode");
    REFUSED(tpl_config_index(p, p, p, 4, 0, 0, 0, big, 0, idx, slot, nullptr), "n_cfg");
    REFUSED(tpl_config_index(p, p, p, 4, 0, 0, 0, 7, -1, idx, slot, nullptr), "n_cfg");
    REFUSED(tpl_config_index(p, p, p, 4, 0, 0, 0, 0, 0, idx, slot, nullptr), "no pool");
    REFUSED(tpl_config_index(p, p, p, 4, 0, 0, 0, 7, 0, nullptr, nullptr, nullptr), "output");
    REFUSED(tpl_config_index(p, p, p, 4, 0, 0, 0, 7, 0, (uint32_t*)odd, slot, nullptr), "4-byte");

    REFUSED(tpl_pool_tally(nullptr, p, p, 4, 2, 3, p, TPL_U8, 0, 0, 0, 7, 0, t, t, nullptr, nullptr, nullptr), "null");
    REFUSED(tpl_pool_tally(p, p, p, 4, 0, 3, p, TPL_U8, 0, 0, 0, 7, 0, t, t, nullptr, nullptr, nullptr), "L and M");
    REFUSED(tpl_pool_tally(p, p, p, 4, 2, 255, p, TPL_U8, 0, 0, 0, 7, 0, t, t, nullptr, nullptr, nullptr), "L and M");
    REFUSED(tpl_pool_tally(p, p, p, 4, 2, 3, nullptr, TPL_U8, 0, 0, 0, 7, 0, t, t, nullptr, nullptr, nullptr), "action");
    REFUSED(tpl_pool_tally(p, p, p, 4, 2, 3, p, 3, 0, 0, 0, 7, 0, t, t, nullptr, nullptr, nullptr), "dtype");
    REFUSED(tpl_pool_tally(p, p, p, 4, 2, 3, odd, TPL_I32, 0, 0, 0, 7, 0, t, t, nullptr, nullptr, nullptr), "aligned");
    REFUSED(tpl_pool_tally(p, p, p, 4, 2, 3, four, TPL_I64, 0, 0, 0, 7, 0, t, t, nullptr, nullptr, nullptr), "aligned");
    REFUSED(tpl_pool_tally(p, p, p, 4, 2, 3, p, TPL_U8, 0, 0, 0, 7, 0, t, nullptr, nullptr, nullptr, nullptr), "go together");
    REFUSED(tpl_pool_tally(p, p, p, 4, 2, 3, p, TPL_U8, 0, 0, 0, 7, 5, t, t, nullptr, t, nullptr), "go together");
    REFUSED(tpl_pool_tally(p, p, p, 4, 2, 3, p, TPL_U8, 0, 0, 0, 7, 0, nullptr, nullptr, nullptr, nullptr, nullptr), "at least one");
    REFUSED(tpl_pool_tally(p, p, p, 4, 2, 3, p, TPL_U8, 0, 0, 0, 7, 0, t, t, t, t, nullptr), "0 entries");
    REFUSED(tpl_pool_tally(p, p, p, 4, 2, 3, p, TPL_U8, 0, 0, 0, 7, 0, (int32_t*)odd, t, nullptr, nullptr, nullptr), "4-byte");
    REFUSED(tpl_pool_tally(p, p, p, 4, 2, 3, p, TPL_U8, 0, 0, 0, 0, 0, t, t, nullptr, nullptr, nullptr), "no pool");

    const int64_t* prefix = (const int64_t*)mem;
    void* out = mem + 128;
    REFUSED(tpl_pool_resample(nullptr, p, 4, 2, prefix, 4, 0, 0, out, out, t, nullptr), "null");
    REFUSED(tpl_pool_resample(p, p, 4, 2, nullptr, 4, 0, 0, out, out, t, nullptr), "null");
    REFUSED(tpl_pool_resample(p, p, 4, 2, prefix, 4, 0, 0, out, out, nullptr, nullptr), "null");
    REFUSED(tpl_pool_resample(p, p, 0, 2, prefix, 4, 0, 0, out, out, t, nullptr), "n_cfg");
    REFUSED(tpl_pool_resample(p, p, (int64_t)1 << 31, 2, prefix, 4, 0, 0, out, out, t, nullptr), "n_cfg");
    REFUSED(tpl_pool_resample(p, p, 4, 2, prefix, 0, 0, 0, out, out, t, nullptr), "count");
    REFUSED(tpl_pool_resample(p, p, 4, 2, prefix, (int64_t)1 << 31, 0, 0, out, out, t, nullptr), "count");
    REFUSED(tpl_pool_resample(p, p, 4, 0, prefix, 4, 0, 0, out, out, t, nullptr), "M must");
    REFUSED(tpl_pool_resample(p, p, 4, 255, prefix, 4, 0, 0, out, out, t, nullptr), "M must");
    REFUSED(tpl_pool_resample(four, p, 4, 2, prefix, 4, 0, 0, out, out, t, nullptr), "8-byte");
    REFUSED(tpl_pool_resample(p, p, 4, 2, (const int64_t*)four, 4, 0, 0, out, out, t, nullptr), "8-byte");
    REFUSED(tpl_pool_resample(p, p, 4, 2, prefix, 4, 0, 0, mem + 132, out, t, nullptr), "8-byte");
    REFUSED(tpl_pool_resample(p, p, 4, 2, prefix, 4, 0, 0, out, out, (int32_t*)odd, nullptr), "4-byte");
    REFUSED(tpl_pool_resample(p, p, 4, 2, prefix, 4, 0, 0, p, out, t, nullptr), "must not be");
    REFUSED(tpl_pool_resample(p, out, 4, 2, prefix, 4, 0, 0, out, out, t, nullptr), "must not be");

    if (g_failed) { printf("%d refusal(s) missing\n", g_failed); return 1; }
    puts("sanitizer run ok");
    return 0;
}
