// adam_host_check.cpp — stand-alone check of csrc/adam_host.hpp under the host sanitizers: pe::adam_bias and pe::train_thread_map (the thread ->
// element map of the persistent training kernel) against the statements they replaced, kept below as they stood inline in engine.cpp, at the
// map's edges and over random row tables.  Nothing of the engine is linked, no device, no Python.  From the repository root:
//   g++ -std=c++17 -g -fsanitize=address,undefined -Ineuralpde.jl_amd/csrc tools/micro/adam_host_check.cpp -o /tmp/adam_host_check && /tmp/adam_host_check
#include "adam_host.hpp"
#include <cassert>
#include <cstdio>
#include <cstring>

// the map as train_common built it before it became a function (G.blocks -> blocks, the PINN_TRAIN_NO_COALESCE read -> !coalesce)
static std::vector<int> parent_map(const std::vector<int>& row_theta, const std::vector<int>& row_ptr, const std::vector<int>& row_off,
                                   int blocks, int P, int K, bool coalesce, int* hist_gid) {
    const int nthr = blocks * 256;
    std::vector<int> own((size_t)nthr, -1);
    bool by_entry = true;
    for (size_t i = 0; i < row_theta.size() && by_entry; ++i) {
        const int e0 = row_ptr[i] < row_ptr[i + 1] ? row_off[row_ptr[i]] : -1;
        if (e0 < 0 || e0 >= nthr - K || own[(size_t)e0] >= 0) by_entry = false;
        else own[(size_t)e0] = row_theta[i];
    }
    int placed = 0;
    for (int v : own) placed += v >= 0;
    if (!by_entry || placed != P || !coalesce) {
        std::fill(own.begin(), own.end(), -1);
        for (int r = 0; r < P; ++r) own[(size_t)r] = r;
    } else {
        int last = 0;
        for (int e = 0; e < nthr; ++e) if (own[(size_t)e] >= 0) last = e;
        const int ngroups = last / 64 + 1;
        if ((ngroups + blocks - 1) / blocks <= 4) {
            std::vector<int> dealt((size_t)nthr, -1);
            for (int g = 0; g < ngroups; ++g)
                for (int l = 0; l < 64; ++l) dealt[(size_t)((g % blocks) * 256 + (g / blocks) * 64 + l)] = own[(size_t)(g * 64 + l)];
            own.swap(dealt);
        }
    }
    for (int k = 0, gid = nthr - 1; k < K && gid >= 0; --gid)
        if (own[(size_t)gid] < 0) own[(size_t)gid] = P + k++;
    *hist_gid = 0;
    for (int gid = nthr - 1; gid >= 0; --gid) if (own[(size_t)gid] < 0) { *hist_gid = gid; break; }
    return own;
}

// row tables of P theta elements whose first slab entries are first[r] (a second entry behind each, as family-1 slabs have several per element)
struct Rows { std::vector<int> theta, ptr, off; };
static Rows rows_from_first(const std::vector<int>& first) {
    Rows R;
    R.ptr.push_back(0);
    for (size_t r = 0; r < first.size(); ++r) {
        R.theta.push_back((int)r);
        if (first[r] != -2) { R.off.push_back(first[r]); R.off.push_back(first[r] + 1000000); }      // (-2: a row without entries)
        R.ptr.push_back((int)R.off.size());
    }
    return R;
}

static int g_cases = 0;
// both builders on one input; the result is also checked for what the kernel relies on: every element of [0, P + K) owned exactly once
static std::vector<int> check(const Rows& R, int blocks, int P, int K, bool coalesce, int* hist_out = nullptr) {
    int ha = -1, hb = -1;
    const std::vector<int> a = pe::train_thread_map(R.theta, R.ptr, R.off, blocks, P, K, coalesce, &ha);
    const std::vector<int> b = parent_map(R.theta, R.ptr, R.off, blocks, P, K, coalesce, &hb);
    assert(a == b && ha == hb);
    assert((int)a.size() == blocks * 256);
    std::vector<int> seen((size_t)(P + K), 0);
    for (int v : a) { assert(v >= -1 && v < P + K); if (v >= 0) ++seen[(size_t)v]; }
    for (int c : seen) assert(c == 1);
    assert(ha >= 0 && ha < blocks * 256 && (a[(size_t)ha] < 0 || ha == 0));
    if (hist_out) *hist_out = ha;
    ++g_cases;
    return a;
}

static unsigned g_rng = 12345u;
static unsigned rnd() { g_rng = g_rng * 1664525u + 1013904223u; return g_rng >> 8; }

int main() {
    // ---- bias corrections: the three statements the function replaced (upload_c12, adam_loop, pinn_adam_apply), bit for bit ----
    const float betas[] = {0.9f, 0.999f, 0.5f, 0.0f, 0.99999f};
    for (float beta : betas)
        for (long long t : {1LL, 2LL, 3LL, 10LL, 1000LL, 4096LL, 100000LL, 123456789LL}) {
            const long long opt_t = t - 1;
            const int s = 0;
            const float parent_table = (float)(1.0 / (1.0 - std::pow((double)beta, (double)(opt_t + s + 1))));
            const float parent_step = (float)(1.0 / (1.0 - std::pow((double)beta, (double)t)));
            const float now = pe::adam_bias(beta, t);
            assert(std::memcmp(&now, &parent_table, sizeof now) == 0 && std::memcmp(&now, &parent_step, sizeof now) == 0);
            assert(now >= 1.0f);
        }
    assert(pe::adam_bias(0.9f, 1) == (float)(1.0 / (1.0 - (double)0.9f)));

    // ---- thread -> element map ----
    int hist = -1;
    {   // blocks = 1, the K sums need every spare thread: P + K == 256, elements placed by entry in a permuted order
        const int P = 250, K = 6;
        std::vector<int> first((size_t)P);
        for (int r = 0; r < P; ++r) first[(size_t)r] = (r * 7) % P;          // distinct, all < 256 - K
        const std::vector<int> own = check(rows_from_first(first), 1, P, K, true, &hist);
        for (int r = 0; r < P; ++r) assert(own[(size_t)first[(size_t)r]] == r);      // (one workgroup: dealing the 64-entry groups changes nothing)
        for (int k = 0; k < K; ++k) assert(own[(size_t)(255 - k)] == P + k);
        assert(hist == 0);                                                    // no thread is left over
    }
    {   // the same with one thread to spare: it becomes hist_gid
        const int P = 249, K = 6;
        std::vector<int> first((size_t)P);
        for (int r = 0; r < P; ++r) first[(size_t)r] = r;
        const std::vector<int> own = check(rows_from_first(first), 1, P, K, true, &hist);
        assert(hist == 249 && own[249] == -1);
    }
    {   // a first-entry collision forces gid = r
        const int P = 100, K = 3;
        std::vector<int> first((size_t)P);
        for (int r = 0; r < P; ++r) first[(size_t)r] = 2 * r;
        first[57] = first[12];
        const std::vector<int> own = check(rows_from_first(first), 1, P, K, true);
        for (int r = 0; r < P; ++r) assert(own[(size_t)r] == r);
        check(rows_from_first(first), 2, P, K, true);
    }
    {   // a first entry inside the last K threads, a row without entries, fewer rows than P, coalescing switched off: gid = r each time
        const int P = 100, K = 4;
        std::vector<int> first((size_t)P);
        for (int r = 0; r < P; ++r) first[(size_t)r] = r;
        std::vector<int> f = first; f[99] = 256 - K;
        std::vector<int> own = check(rows_from_first(f), 1, P, K, true);
        assert(own[99] == 99 && own[252] == P + 3);
        f[99] = 256 - K - 1;                                                  // the last admissible entry: placed by entry
        own = check(rows_from_first(f), 1, P, K, true);
        assert(own[251] == 99 && own[99] == -1);
        f = first; f[40] = -2;
        own = check(rows_from_first(f), 1, P, K, true);
        assert(own[40] == 40);
        f = first; f.pop_back();                                              // 99 rows for P = 100
        own = check(rows_from_first(f), 1, P, K, true);
        assert(own[99] == 99);
        f = first; for (int r = 0; r < P; ++r) f[(size_t)r] = P - 1 - r;
        own = check(rows_from_first(f), 1, P, K, false);
        assert(own[0] == 0);
        own = check(rows_from_first(f), 1, P, K, true);
        assert(own[0] == P - 1);
    }
    {   // several workgroups: 64-entry groups dealt round-robin.  ngroups = last / 64 + 1 with last < 256 blocks - K, so ngroups <= 4 blocks
        // always holds: "just under" and "at" the limit are the edges that exist (4 blocks - 1 and 4 blocks groups); beyond it the first
        // entry is refused before the deal
        for (int blocks : {2, 3, 5, 32}) {
            for (int top : {256 * blocks - 64 - 1, 256 * blocks - 64, 256 * blocks - 1}) {        // last entry in group 4 blocks - 2 / - 1 / - 1
                const int K = top == 256 * blocks - 1 ? 0 : 5, P = 300;
                if (top >= 256 * blocks - K || P + K > 256 * blocks) continue;
                std::vector<int> first((size_t)P);
                for (int r = 0; r < P; ++r) first[(size_t)r] = r;
                first[(size_t)(P - 1)] = top;
                const std::vector<int> own = check(rows_from_first(first), blocks, P, K, true);
                const int g = top / 64, l = top % 64;
                assert(own[(size_t)((g % blocks) * 256 + (g / blocks) * 64 + l)] == P - 1);
                assert(own[(size_t)((1 % blocks) * 256 + (1 / blocks) * 64 + 3)] == 67);          // entry 67 = group 1, lane 3
            }
        }
    }
    // random row tables: distinct / colliding / out-of-range first entries, every blocks in 1..6, K in 0..8
    for (int it = 0; it < 3000; ++it) {
        const int blocks = 1 + (int)(rnd() % 6), K = (int)(rnd() % 9), nthr = blocks * 256;
        const int P = 1 + (int)(rnd() % (unsigned)(nthr - K));
        std::vector<int> perm((size_t)nthr);
        for (int e = 0; e < nthr; ++e) perm[(size_t)e] = e;
        const int span = std::max(P, 1 + (int)(rnd() % (unsigned)nthr));     // first entries drawn from [0, span)
        for (int e = span - 1; e > 0; --e) std::swap(perm[(size_t)e], perm[(size_t)(rnd() % (unsigned)(e + 1))]);
        std::vector<int> first(perm.begin(), perm.begin() + P);
        const unsigned kind = rnd() % 4;
        if (kind == 1) first[(size_t)(rnd() % (unsigned)P)] = first[(size_t)(rnd() % (unsigned)P)];       // maybe a collision
        if (kind == 2) first[(size_t)(rnd() % (unsigned)P)] = -2;
        check(rows_from_first(first), blocks, P, K, rnd() % 8 != 0);
    }
    std::printf("adam_host: ok (%d map cases)\n", g_cases);
    return 0;
}
