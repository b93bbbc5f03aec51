// partition_host_check.cpp -- a stand-alone program over the host-compilable half of the batched region partition
// (safelife_amd/csrc/sl_partition_core.h): the launch's argument validation and workspace sizing, the state layout, the
// bounded draw, the region pick, and the partition itself, run on the CPU through the very functions the kernel calls, put
// together the way the kernel puts them together.  tests/test_partition_host.py builds it with -fsanitize=address,undefined
// and runs it; every partition's state lives in a heap block of EXACTLY Layout.bytes, so an index outside the state is an
// AddressSanitizer report here instead of a stray write on a GPU.
//
//   partition_host_check                 the self-checks
//   partition_host_check CASES.bin       the self-checks, then every case of the file (written by the test from
//                                        proc_gen.partition): status, labels and generator words must come out as recorded
// Exit status 0: everything held.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../safelife_amd/csrc/sl_partition_core.h"

using namespace sl::pt;

static int g_failed = 0;
#define CHECK(cond)                                                             \
    do {                                                                        \
        if (!(cond)) {                                                          \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);       \
            g_failed++;                                                         \
        }                                                                       \
    } while (0)

struct Result {
    std::vector<int16_t> labels;        // empty unless status is 0
    u64 words[6];
    int status, turns, regions;
};

// one problem as a workgroup of the kernel runs it, `lanes` "lanes" sharing the loops (64: the ballots as the wavefront
// forms them; 1: everything one after the other); `room`: the regions the state has room for
static Result run_partition(int rows, int cols, int room, int min_regions, int max_regions, const u64 *words, int lanes) {
    Result res;
    std::memcpy(res.words, words, sizeof res.words);
    res.turns = res.regions = 0;
    int lo, hi;
    clamp_bounds(min_regions, max_regions, lo, hi);
    if (!shape_ok(rows, cols) || hi > room) {
        res.status = STATUS_REFUSED;
        return res;
    }
    const Layout l = make_layout(rows, cols, room);
    unsigned char *state = (unsigned char *)std::malloc(l.bytes);
    std::memset(state, 0xA5, l.bytes);
    const View v = make_view(state, l);
    Run run = {};
    for (int lane = 0; lane < lanes; lane++) init_clear(v, l.regions, lane, lanes);
    begin(v, run, words, lo, hi);
    const int want = v.ctrl->done ? 0 : v.ctrl->want;
    for (int k = 1; k <= want; k++) {
        int count = 0;
        for (int chunk = 0; chunk < v.words; chunk++) {
            u64 free = 0;
            for (int lane = 0; lane < WAVE; lane++) {
                const int cell = chunk * WAVE + lane;
                if (cell < v.cells && seed_free(v, cell, k)) free |= 1ull << lane;
            }
            v.queued[(size_t)(k - 1) * v.words + chunk] = free;
            count += __builtin_popcountll(free);
        }
        if (!count) break;
        seed_take(v, run, k, count);
        if (v.ctrl->done) break;
    }
    for (;;) {
        turn_head(v, run);
        if (v.ctrl->done) break;
        const int cell = v.ctrl->cell, k = v.ctrl->k;
        const int r = cell / v.cols, c = cell - r * v.cols;
        bool blocked = false;
        for (int lane = NEAR - 1; lane >= 0; lane--) blocked |= near_blocked(v, r, c, k + 1, lane);     // any order
        if (!blocked) turn_tail(v, run);
    }
    res.status = v.ctrl->status;
    res.turns = run.turns;
    res.regions = v.ctrl->n_regions;
    if (res.status == STATUS_OK) {
        res.labels.assign(v.label, v.label + v.cells);
        store_words(run.rng, res.words);
    }
    std::free(state);
    return res;
}

static bool same(const Result &a, const Result &b) {
    return a.status == b.status && a.labels == b.labels && !std::memcmp(a.words, b.words, sizeof a.words);
}

static void check_validation() {
    alignas(16) static unsigned char buf[64];
    const char *why = nullptr;
    const void *p = buf;
#define V(n, room, need, ws, wsz) validate(p, p, p, p, p, n, room, need, ws, wsz, &why)
    CHECK(V(1, 3, 0, nullptr, 0) == E_OK);
    CHECK(V(0, 3, 0, nullptr, 0) == E_OK);
    CHECK(V(-1, 3, 0, nullptr, 0) == E_ARG);
    CHECK(V(1, 0, 0, nullptr, 0) == E_ARG && V(1, 9, 0, nullptr, 0) == E_ARG);
    const size_t need = workspace_bytes(3, 64, 64, 8);
    CHECK(need == 3 * (size_t)make_layout(64, 64, 8).bytes && need > 3 * (size_t)LDS_LIMIT);
    CHECK(V(3, 8, need, nullptr, 0) == E_ARG);
    CHECK(V(3, 8, need, p, need - 1) == E_ARG);
    CHECK(V(3, 8, need, p, need) == E_OK);
    CHECK(V(3, 8, need, buf + 8, need) == E_ARG);
#undef V
    CHECK(validate(nullptr, p, p, p, p, 1, 3, 0, nullptr, 0, &why) == E_ARG);
    CHECK(validate(buf + 4, p, p, p, p, 1, 3, 0, nullptr, 0, &why) == E_ARG);
    CHECK(validate(p, buf + 2, p, p, p, 1, 3, 0, nullptr, 0, &why) == E_ARG);
    CHECK(validate(p, p, p, buf + 1, p, 1, 3, 0, nullptr, 0, &why) == E_ARG);
    CHECK(validate(p, p, p, p, p, 1, 3, 0, nullptr, 0, nullptr) == E_OK);
    // sizing: nothing for what is refused anyway, nothing where the state fits LDS
    CHECK(workspace_bytes(0, 64, 64, 8) == 0 && workspace_bytes(5, 2, 26, 3) == 0 && workspace_bytes(5, 26, 65, 3) == 0);
    CHECK(workspace_bytes(5, 64, 64, 9) == 0 && workspace_bytes(5, 64, 64, 0) == 0);
    CHECK(workspace_bytes(5, 26, 26, 8) == 0 && workspace_bytes(5, 64, 64, 7) == 0 && workspace_bytes(5, 63, 61, 8) > 0);
}

static void check_layouts() {
    for (int room = 1; room <= MAX_REGIONS; room++)
        for (int rows = MIN_SIDE; rows <= MAX_SIDE; rows += (rows < 8 ? 1 : 7))
            for (int cols = MIN_SIDE; cols <= MAX_SIDE; cols += (cols < 8 ? 1 : 19)) {
                const Layout l = make_layout(rows, cols, room);
                const unsigned off[] = {l.off_ctrl, l.off_queued, l.off_frontier, l.off_label, l.bytes};
                const unsigned size[] = {(unsigned)sizeof(Ctrl), 8u * room * l.words, 2u * room * l.cells, 1u * l.cells};
                for (int k = 0; k < 4; k++) CHECK(off[k] + size[k] <= off[k + 1]);
                CHECK(l.off_ctrl % 8 == 0 && l.off_queued % 8 == 0 && l.off_frontier % 2 == 0 && l.bytes % 16 == 0);
                CHECK(l.words * 64 >= l.cells && (l.words - 1) * 64 < l.cells && l.cells <= 4096);
                CHECK((workspace_bytes(2, rows, cols, room) == 0) == (l.bytes <= LDS_LIMIT));
            }
    CHECK(make_layout(26, 26, 3).bytes <= 5120 && make_layout(26, 26, 5).bytes <= 8192);     // what the kernel's comment promises
    CHECK(make_layout(64, 64, 8).bytes > LDS_LIMIT && make_layout(64, 64, 8).bytes <= 73 * 1024);
}

static void check_wrap() {
    for (int n = MIN_SIDE; n <= MAX_SIDE; n++)
        for (int x = -2; x <= n + 1; x++) CHECK(wrap(x, n) == ((x % n) + n) % n);
}

// the bounded draw against its definition, the n == 1 case, and the cap
static void check_bounded() {
    Rng g = {1, 2, 0, 7, 0, 0};
    const Rng before = g;
    uint32_t out = 99;
    CHECK(bounded(g, 1, out) && out == 0 && !std::memcmp(&g, &before, sizeof g));         // nothing drawn
    for (uint32_t n = 2; n < 5000; n += (n < 70 ? 1 : 131)) {
        Rng a = g, b = g;
        CHECK(bounded(a, n, out) && out < n);
        u64 m;
        do {
            m = (u64)sl::gp::next32(b) * n;
        } while ((uint32_t)m < (0x100000000ull - n) % n);
        CHECK(out == (uint32_t)(m >> 32) && !std::memcmp(&a, &b, sizeof a));
        g = a;
    }
    // n = 2^31 + 1 redraws about every other time, the worst there is: 64 redraws in a row (2^-64) still do not happen
    int capped = 0;
    for (int i = 0; i < 2000; i++) {
        if (!bounded(g, 0x80000001u, out)) capped++;
        else CHECK(out < 0x80000001u);
    }
    CHECK(capped == 0);
}

// the region pick with crafted `at` values: the plain cases, the empty regions in front, and the fall-back when the walk
// ends on an empty last region (at == total after rounding)
static void check_pick() {
    const int a[] = {3, 0, 2};
    CHECK(pick_region(a, 3, 0.0) == 0 && pick_region(a, 3, 2.999) == 0);
    CHECK(pick_region(a, 3, 3.0) == 2 && pick_region(a, 3, 4.999) == 2 && pick_region(a, 3, 5.0) == 2);
    const int b[] = {0, 0, 4, 0};
    CHECK(pick_region(b, 4, 0.0) == 2 && pick_region(b, 4, 3.9) == 2);
    CHECK(pick_region(b, 4, 4.0) == 2);                 // walks to the empty last region, falls back round to region 2
    const int c[] = {5, 0};
    CHECK(pick_region(c, 2, 4.9) == 0 && pick_region(c, 2, 5.0) == 0);      // the same, wrapping from the end to the front
    const int d[] = {0, 0, 0, 7};
    CHECK(pick_region(d, 4, 6.5) == 3 && pick_region(d, 4, 7.0) == 3);
    const int e[] = {4};
    CHECK(pick_region(e, 1, 0.0) == 0 && pick_region(e, 1, 4.0) == 0);
    const int z[] = {0, 0};
    CHECK(pick_region(z, 2, 0.0) >= 0 && pick_region(z, 2, 0.0) < 2);       // never asked (total is 0), but it ends
    // the subtraction is a double's: one rounding per step
    const int f[] = {1, 1, 1};
    CHECK(pick_region(f, 3, 0x1.fffffffffffffp+0) == 1 && pick_region(f, 3, 2.0) == 2);
}

// made-up problems at the shapes where an index could go wrong; serial against 64 lanes; properties of the result
static void check_synthetic() {
    const int shapes[][4] = {{3, 3, 1, 3}, {3, 3, 8, 8}, {3, 64, 2, 4}, {64, 3, 1, 5}, {4, 5, 2, 2}, {5, 5, 2, 5}, {7, 6, 2, 8},
                             {8, 8, 1, 1}, {13, 20, 2, 4}, {26, 26, 2, 3}, {26, 26, 1, 1}, {63, 61, 3, 5}, {64, 64, 8, 8},
                             {64, 64, 1, 1}};
    u64 lcg = 4321;
    for (const auto &s : shapes)
        for (int rep = 0; rep < 3; rep++) {
            lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
            const int rows = s[0], cols = s[1], cells = rows * cols;
            const u64 words[6] = {lcg, lcg ^ 0x9E3779B97F4A7C15ull, (u64)rep, (lcg << 1) | 1, (u64)(rep & 1), 0xDEADBEEF};
            const Result a = run_partition(rows, cols, s[3], s[2], s[3], words, 1);
            const Result b = run_partition(rows, cols, MAX_REGIONS, s[2], s[3], words, 64);     // more room, same result
            CHECK(a.status == STATUS_OK && same(a, b));
            if (a.status != STATUS_OK) continue;
            CHECK(a.regions >= 1 && a.regions <= s[3] && a.turns <= a.regions * cells + 1);
            int taken = 0;
            for (int i = 0; i < cells; i++) {
                CHECK(a.labels[i] >= 0 && a.labels[i] <= a.regions);
                taken += a.labels[i] != 0;
                for (int lane = 0; lane < NEAR && a.labels[i]; lane++) {        // regions keep two cells apart
                    const int other = a.labels[wrap(i / cols + lane / 5 - 2, rows) * cols + wrap(i % cols + lane % 5 - 2, cols)];
                    CHECK(!other || other == a.labels[i]);
                }
            }
            if (a.regions == 1) CHECK(taken <= (4 * cells) / 5 || taken == 1);
        }
    // refusals: nothing drawn, nothing written
    const u64 words[6] = {1, 2, 3, 5, 1, 77};
    const int bad[][5] = {{2, 26, 8, 2, 3}, {26, 2, 8, 2, 3}, {65, 26, 8, 2, 3}, {26, 65, 8, 2, 3}, {26, 26, 8, 2, 9},
                          {26, 26, 8, 9, 1}, {26, 26, 3, 2, 4}, {26, 26, 8, 100, -5}};
    for (const auto &s : bad) {
        const Result r = run_partition(s[0], s[1], s[2], s[3], s[4], words, 64);
        CHECK(r.status == STATUS_REFUSED && r.labels.empty() && !std::memcmp(r.words, words, sizeof words));
    }
    // clamping: min below 1 and max below min
    int lo, hi;
    clamp_bounds(-3, 0, lo, hi);
    CHECK(lo == 1 && hi == 1);
    clamp_bounds(4, 2, lo, hi);
    CHECK(lo == 4 && hi == 4);
    clamp_bounds(2, 5, lo, hi);
    CHECK(lo == 2 && hi == 5);
}

static bool read_exact(std::FILE *f, void *dst, size_t n) { return std::fread(dst, 1, n, f) == n; }

static void check_cases(const char *path) {
    std::FILE *f = std::fopen(path, "rb");
    if (!f) {
        std::printf("cannot open %s\n", path);
        g_failed++;
        return;
    }
    int32_t n = 0;
    CHECK(read_exact(f, &n, 4));
    for (int k = 0; k < n && !g_failed; k++) {
        int32_t head[5];            // rows, cols, min_regions, max_regions, room
        u64 w0[6], w1[6];
        CHECK(read_exact(f, head, sizeof head) && read_exact(f, w0, sizeof w0) && read_exact(f, w1, sizeof w1));
        const int rows = head[0], cols = head[1];
        CHECK(shape_ok(rows, cols));
        if (g_failed) break;
        std::vector<int16_t> want((size_t)rows * cols);
        CHECK(read_exact(f, want.data(), want.size() * 2));
        for (int lanes = 1; lanes <= 64; lanes += 63) {
            const Result r = run_partition(rows, cols, head[4], head[2], head[3], w0, lanes);
            const bool ok = r.status == STATUS_OK && r.labels == want && !std::memcmp(r.words, w1, 48);
            if (!ok) {
                std::printf("case %d (%dx%d, regions %d..%d, room %d, lanes %d): status %d, labels %s, words %s\n", k, rows, cols,
                            head[2], head[3], head[4], lanes, r.status, r.labels == want ? "equal" : "DIFFER",
                            std::memcmp(r.words, w1, 48) ? "DIFFER" : "equal");
                g_failed++;
            }
        }
    }
    std::fclose(f);
    std::printf("%d recorded cases\n", n);
}

int main(int argc, char **argv) {
    check_validation();
    check_layouts();
    check_wrap();
    check_bounded();
    check_pick();
    check_synthetic();
    if (argc > 1) check_cases(argv[1]);
    std::printf(g_failed ? "%d checks FAILED\n" : "all checks held\n", g_failed);
    return g_failed ? 1 : 0;
}
