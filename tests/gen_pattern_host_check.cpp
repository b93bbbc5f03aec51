// gen_pattern_host_check.cpp -- a stand-alone program over the host-compilable half of the pattern generator
// (safelife_amd/csrc/sl_gen_pattern_core.h): the launch's argument validation and workspace sizing, the state layout, and
// the chain itself, run on the CPU through the very functions the kernel calls.  tests/test_gen_pattern_host.py builds it
// with -fsanitize=address,undefined and runs it; every chain's state lives in a heap block of EXACTLY Layout.bytes, so an
// index outside the state is an AddressSanitizer report here instead of a stray write on a GPU.
//
//   gen_pattern_host_check                 the self-checks
//   gen_pattern_host_check CASES.bin       the self-checks, then every recorded case of the file (written by the test from
//                                          tests/golden/gen_pattern_cases.npz): board, status and generator words must come
//                                          out as recorded, walking the candidates one by one AND (depth 1) slot by slot
// Exit status 0: everything held.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../safelife_amd/csrc/sl_gen_pattern_core.h"

using namespace sl::gp;

static int g_failed = 0;
#define CHECK(cond)                                                             \
    do {                                                                        \
        if (!(cond)) {                                                          \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);       \
            g_failed++;                                                         \
        }                                                                       \
    } while (0)

struct Result {
    std::vector<uint16_t> board;
    u64 words[6];
    int status, iterations;
};

// one chain; `slots`: depth-1 candidates slot by slot as the wavefront's lanes take them (else one by one with swaps);
// `lanes`: how many "lanes" share the set-up loops
static Result run_chain(int rows, int cols, int depth, const uint16_t *layers, const int32_t *mask, const int32_t *seeds,
                        const double *params, const u64 *words, bool slots, int lanes) {
    const Layout l = make_layout(rows, cols, depth);
    unsigned char *state = (unsigned char *)std::malloc(l.bytes);
    std::memset(state, 0xA5, l.bytes);
    const View v = make_view(state, l);
    Chain ch = {};
    for (int lane = 0; lane < lanes; lane++) init_copy(v, layers, mask, lane, lanes);
    for (int lane = 0; lane < lanes; lane++) init_counts(v, lane, lanes);
    init_sets(v, ch, mask, seeds, params, words);
    for (;;) {
        iter_head(v, ch, params);
        if (v.ctrl->done) break;
        int num;
        if (slots && depth == 1) {
            for (int slot = 26; slot >= 0; slot--) candidate_depth1(v, slot);     // any order: the slots are independent
            num = compact_depth1(v);
        } else {
            num = candidates_serial(v);
        }
        iter_tail(v, ch, num);
    }
    Result r;
    r.status = chain_status(ch);
    r.iterations = ch.it;
    const uint16_t *src = r.status == STATUS_OK ? v.board : layers;
    r.board.assign(src, src + l.layer);
    const u64 w[6] = {ch.rng.hi, ch.rng.lo, ch.rng.inc_hi, ch.rng.inc_lo, ch.rng.has_uint32, ch.rng.uinteger};
    std::memcpy(r.words, w, sizeof w);
    std::free(state);
    return r;
}

static bool same(const Result &a, const Result &b) {
    return a.status == b.status && a.iterations == b.iterations && a.board == b.board &&
           !std::memcmp(a.words, b.words, sizeof a.words);
}

static void check_validation() {
    alignas(16) static unsigned char buf[64];
    const char *why = nullptr;
    const void *p = buf;
#define V(n, h, w, d, ws, wsz) validate(p, p, p, p, p, p, p, n, h, w, d, ws, wsz, &why)
    CHECK(V(1, 3, 3, 1, nullptr, 0) == E_OK);
    CHECK(V(1, 48, 48, 1, nullptr, 0) == E_OK);
    CHECK(V(1, 64, 64, 1, nullptr, 0) == E_ARG);                // 4096 cells: the state is over 64 KiB, a workspace it is
    CHECK(V(0, 3, 3, 1, nullptr, 0) == E_OK);
    CHECK(V(-1, 3, 3, 1, nullptr, 0) == E_ARG);
    CHECK(V(1, 2, 3, 1, nullptr, 0) == E_SHAPE && !std::strcmp(why, "Board must be at least 3x3."));
    CHECK(V(1, 3, 2, 1, nullptr, 0) == E_SHAPE);
    CHECK(V(1, 3, 3, 0, nullptr, 0) == E_ARG && !std::strcmp(why, "Pattern period must be larger than 0."));
    CHECK(V(1, 65, 3, 1, nullptr, 0) == E_UNSUPPORTED);
    CHECK(V(1, 3, 65, 1, nullptr, 0) == E_UNSUPPORTED);
    CHECK(V(1, 3, 3, 5, nullptr, 0) == E_UNSUPPORTED);
    // a shape that needs the workspace
    const size_t need = workspace_bytes(3, 64, 64, 4);
    CHECK(need == 3 * (size_t)make_layout(64, 64, 4).bytes && need > 0);
    CHECK(V(3, 64, 64, 4, nullptr, 0) == E_ARG);
    CHECK(V(3, 64, 64, 4, p, need - 1) == E_ARG);
    CHECK(V(3, 64, 64, 4, p, need) == E_OK);
    CHECK(V(3, 64, 64, 4, buf + 8, need) == E_ARG);
#undef V
    CHECK(validate(nullptr, p, p, p, p, p, p, 1, 3, 3, 1, nullptr, 0, &why) == E_ARG);
    CHECK(validate(p, p, buf + 4, p, p, p, p, 1, 3, 3, 1, nullptr, 0, &why) == E_ARG);
    CHECK(validate(p, p, p, p, buf + 1, p, p, 1, 3, 3, 1, nullptr, 0, &why) == E_ARG);
    CHECK(validate(p, p, p, p, p, p, p, 1, 3, 3, 1, nullptr, 0, nullptr) == E_OK);
    CHECK(workspace_bytes(0, 26, 26, 1) == 0 && workspace_bytes(5, 2, 26, 1) == 0 && workspace_bytes(5, 26, 26, 9) == 0);
}

static void check_layouts() {
    for (int depth = 1; depth <= MAX_DEPTH; depth++)
        for (int rows = MIN_SIDE; rows <= MAX_SIDE; rows += (rows < 8 ? 1 : 7))
            for (int cols = MIN_SIDE; cols <= MAX_SIDE; cols += (cols < 8 ? 1 : 19)) {
                const Layout l = make_layout(rows, cols, depth);
                const unsigned off[] = {l.off_lp, l.off_ctrl, l.off_board, l.off_sets, l.off_ctype, l.off_cidx,
                                        l.off_nbr, l.off_viol, l.off_osc, l.off_mask, l.bytes};
                const unsigned size[] = {8u * l.cand, (unsigned)sizeof(Ctrl), 2u * depth * l.layer, 12u * l.layer, 2u * l.cand,
                                         2u * l.cand, 1u * depth * l.layer, 1u * l.layer, 1u * l.layer, 1u * l.layer};
                for (int k = 0; k < 10; k++) CHECK(off[k] + size[k] <= off[k + 1]);
                CHECK(l.off_lp % 8 == 0 && l.off_ctrl % 8 == 0 && l.off_board % 2 == 0 && l.off_sets % 2 == 0 &&
                      l.off_ctype % 2 == 0 && l.off_cidx % 2 == 0 && l.bytes % 16 == 0);
                CHECK((workspace_bytes(2, rows, cols, depth) == 0) == (l.bytes <= LDS_LIMIT));
                CHECK(l.layer <= 4096 && l.layer < NO_CANDIDATE);
            }
    CHECK(make_layout(26, 26, 1).bytes <= 16384);        // what the kernel's header comment promises
    CHECK(make_layout(48, 48, 1).bytes <= LDS_LIMIT && make_layout(26, 26, 4).bytes <= LDS_LIMIT);
}

// made-up problems at the shapes where an index could go wrong: the smallest, narrow against the window, the largest
static void check_synthetic() {
    const int shapes[][3] = {{3, 3, 1}, {3, 3, 2}, {3, 3, 4}, {4, 5, 3}, {3, 64, 2}, {64, 3, 1}, {7, 11, 1}, {26, 26, 1},
                             {26, 26, 2}, {64, 64, 1}, {64, 64, 4}};
    u64 lcg = 12345;
    for (const auto &s : shapes) {
        const int rows = s[0], cols = s[1], depth = s[2], layer = rows * cols;
        std::vector<uint16_t> layers((size_t)depth * layer, 0);
        std::vector<int32_t> mask(layer), seeds(layer);
        for (int i = 0; i < layer; i++) {
            lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
            const unsigned x = (unsigned)(lcg >> 33);
            mask[i] = (x % 11 == 0) ? 4 : (x % 13 == 0) ? 0 : (x % 7 == 0) ? 5 : 7;
            seeds[i] = (x % 5 == 0);
            for (int d = 0; d < depth; d++) layers[(size_t)d * layer + i] = (x % 17 == 0) ? 16 : (x % 19 == 0) ? 9 : 0;
        }
        const double iters = depth == 1 ? 300.0 : 40.0;
        double params[12] = {iters / (layer * depth), 0.2, 0.7, 0.3, 0, 0, 2, 3, 0, 1, 3, 2};
        const u64 words[6] = {lcg, lcg ^ 0x9E3779B97F4A7C15ull, 0, (lcg << 1) | 1, 1, 0xDEADBEEF};
        const Result a = run_chain(rows, cols, depth, layers.data(), mask.data(), seeds.data(), params, words, false, 1);
        const Result b = run_chain(rows, cols, depth, layers.data(), mask.data(), nullptr, params, words, true, 64);
        const Result c = run_chain(rows, cols, depth, layers.data(), mask.data(), seeds.data(), params, words, true, 64);
        CHECK(same(a, c));
        CHECK(b.status == STATUS_OK || b.status == STATUS_MAX_ITER);
        params[0] = 1e300;                                      // the limit does not fit an int: refused, nothing drawn
        const Result d = run_chain(rows, cols, depth, layers.data(), mask.data(), seeds.data(), params, words, true, 64);
        CHECK(d.status == STATUS_REFUSED && d.iterations == 0 && !std::memcmp(d.words, words, sizeof words));
    }
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
        int32_t head[6];            // rows, cols, depth, has_seeds, status, iterations
        double params[12];
        u64 w0[6], w1[6];
        CHECK(read_exact(f, head, sizeof head) && read_exact(f, params, sizeof params) && read_exact(f, w0, sizeof w0) &&
              read_exact(f, w1, sizeof w1));
        const int rows = head[0], cols = head[1], depth = head[2], layer = rows * cols;
        CHECK(shape_ok(rows, cols, depth));
        if (g_failed) break;
        std::vector<uint16_t> layers((size_t)depth * layer), want(layer);
        std::vector<int32_t> mask(layer), seeds(layer);
        CHECK(read_exact(f, layers.data(), layers.size() * 2) && read_exact(f, mask.data(), mask.size() * 4));
        if (head[3]) CHECK(read_exact(f, seeds.data(), seeds.size() * 4));
        CHECK(read_exact(f, want.data(), want.size() * 2));
        for (int slots = 0; slots < 2; slots++) {
            const Result r = run_chain(rows, cols, depth, layers.data(), mask.data(), head[3] ? seeds.data() : nullptr, params,
                                       w0, slots != 0, slots ? 64 : 1);
            const bool ok = r.status == head[4] && r.iterations == head[5] && r.board == want && !std::memcmp(r.words, w1, 48);
            if (!ok) {
                std::printf("case %d (%dx%d depth %d, slots %d): status %d want %d, iterations %d want %d, board %s, words %s\n",
                            k, rows, cols, depth, slots, r.status, head[4], r.iterations, head[5],
                            r.board == want ? "equal" : "DIFFER", std::memcmp(r.words, w1, 48) ? "DIFFER" : "equal");
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
    check_synthetic();
    if (argc > 1) check_cases(argv[1]);
    std::printf(g_failed ? "%d checks FAILED\n" : "all checks held\n", g_failed);
    return g_failed ? 1 : 0;
}
