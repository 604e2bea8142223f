// deflate_huff.cpp — the device DEFLATE encoder's Huffman routines (svim_asm_amd/csrc/svx_deflate_huff.h: build_lengths,
// make_codes, rle_lengths) compiled for the host and checked against references written here:
//   * plain Huffman by repeated extraction of the minimum, 64-bit weights, ties to the shallower subtree — the optimal
//     cost and the SMALLEST depth an optimal code can have (Schwartz 1964), which is also what a two-queue build that
//     prefers leaves on ties reaches;
//   * package-merge (Larmore & Hirschberg 1990) for the optimal cost under a length limit;
//   * RFC 1951 §3.2.2's code assignment, bit by bit.
// Frequency vectors are what one block can produce (every used symbol >= 1, sum <= 65 281) and are aimed at the length
// limiter: Fibonacci runs (depth k - 1 over k symbols), permuted and tied, geometric, one huge symbol over singletons,
// seeded random supports and skews.  Built with -fsanitize=address,undefined by tests/test_deflate_huff.py; the work
// areas live on the heap at their exact sizes.  Usage: deflate_huff [random vectors per alphabet] [seed]
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "svx_deflate_huff.h"

namespace {

constexpr uint64_t kMaxSum = 65281;  // 65 280 literals at the most, and the end-of-block symbol

int g_fail = 0;
void fail(const std::string& what, const char* alpha, const std::string& name) {
    if (++g_fail <= 20) std::printf("FAIL [%s] %s: %s\n", alpha, name.c_str(), what.c_str());
}

struct Ref {
    uint64_t cost;   // sum f * len of an optimal prefix code
    int depth;       // the smallest maximum length among the optimal codes
};

// Huffman's algorithm as stated: take the two smallest, put their sum back.  Ties go to the shallower subtree.
Ref huffman_ref(const std::vector<uint64_t>& used) {
    std::vector<std::pair<uint64_t, int>> q;
    for (uint64_t f : used) q.push_back({f, 0});
    uint64_t cost = 0;
    while (q.size() > 1) {
        std::pair<uint64_t, int> two[2];
        for (auto& t : two) {
            auto it = std::min_element(q.begin(), q.end());
            t = *it;
            q.erase(it);
        }
        cost += two[0].first + two[1].first;  // every merge adds one bit to each leaf below it
        q.push_back({two[0].first + two[1].first, std::max(two[0].second, two[1].second) + 1});
    }
    return {cost, q.empty() ? 0 : q[0].second};
}

// package-merge: the cost of an optimal code whose lengths are all <= limit (needs used.size() <= 2^limit)
uint64_t package_merge_cost(std::vector<uint64_t> used, int limit) {
    std::sort(used.begin(), used.end());
    const size_t m = used.size();
    std::vector<uint64_t> cur = used;
    for (int level = 1; level < limit; ++level) {
        std::vector<uint64_t> merged;
        for (size_t k = 0; k + 1 < cur.size(); k += 2) merged.push_back(cur[k] + cur[k + 1]);
        merged.insert(merged.end(), used.begin(), used.end());
        std::stable_sort(merged.begin(), merged.end());
        cur.swap(merged);
    }
    uint64_t cost = 0;
    for (size_t k = 0; k < 2 * m - 2; ++k) cost += cur[k];
    return cost;
}

uint32_t reverse_bits(uint32_t v, int n) {
    uint32_t r = 0;
    for (int i = 0; i < n; ++i) r |= ((v >> i) & 1u) << (n - 1 - i);
    return r;
}

struct Alphabet {
    const char* name = "";
    int n = 0, maxbits = 0;
    uint64_t vectors = 0, limited = 0, at_limit = 0;
    double worst = 1.0;
    std::string worst_name;
};

void check(Alphabet& A, const std::vector<uint32_t>& f, const std::string& name) {
    const int n = A.n, maxbits = A.maxbits;
    // exact sizes on the heap: a write past any of them is the sanitizer's to report
    std::unique_ptr<uint32_t[]> freq(new uint32_t[n]);
    std::unique_ptr<uint8_t[]> len(new uint8_t[n]);
    std::unique_ptr<uint16_t[]> code(new uint16_t[n]);
    std::unique_ptr<HuffWork> hw(new HuffWork);
    std::memcpy(freq.get(), f.data(), 4 * (size_t)n);
    std::memset(len.get(), 0xEE, (size_t)n);
    std::memset(hw.get(), 0xEE, sizeof(HuffWork));
    build_lengths(freq.get(), n, maxbits, len.get(), *hw);
    ++A.vectors;

    std::vector<uint64_t> used;
    std::vector<int> used_sym;
    for (int i = 0; i < n; ++i)
        if (f[i]) { used.push_back(f[i]); used_sym.push_back(i); }
    // which symbols must carry a code: the used ones, and with fewer than two of them symbols 0 / 1 (zlib's rule)
    std::vector<char> coded(n, 0);
    for (int s : used_sym) coded[s] = 1;
    if (used.size() == 0) coded[0] = coded[1] = 1;
    if (used.size() == 1) coded[used_sym[0] == 0 ? 1 : 0] = 1;
    uint64_t kraft = 0, cost = 0;
    for (int i = 0; i < n; ++i) {
        if (!coded[i]) {
            if (len[i] != 0) fail("unused symbol " + std::to_string(i) + " has length " + std::to_string(len[i]), A.name, name);
            continue;
        }
        if (len[i] < 1 || len[i] > maxbits) {
            fail("symbol " + std::to_string(i) + " has length " + std::to_string(len[i]), A.name, name);
            return;
        }
        kraft += 1ull << (maxbits - len[i]);
        cost += (uint64_t)f[i] * len[i];
    }
    if (kraft != 1ull << maxbits) fail("Kraft sum " + std::to_string(kraft) + " / " + std::to_string(1ull << maxbits), A.name, name);
    if (used.size() < 2) {
        for (int i = 0; i < n; ++i)
            if (coded[i] && len[i] != 1) fail("fewer than two used symbols: length " + std::to_string(len[i]) + " instead of 1", A.name, name);
    } else {
        const Ref ref = huffman_ref(used);
        const uint64_t opt = package_merge_cost(used, maxbits);
        // the references against each other: the limit costs nothing exactly where an optimal code fits under it
        if ((ref.depth <= maxbits) != (opt == ref.cost) || opt < ref.cost)
            fail("references disagree: depth " + std::to_string(ref.depth) + ", Huffman " + std::to_string(ref.cost) +
                 ", package-merge " + std::to_string(opt), A.name, name);
        if (ref.depth == maxbits) ++A.at_limit;
        if (ref.depth <= maxbits) {
            if (cost != ref.cost) fail("cost " + std::to_string(cost) + " where the optimum " + std::to_string(ref.cost) +
                                       " fits the limit (depth " + std::to_string(ref.depth) + ")", A.name, name);
        } else {
            ++A.limited;
            if (cost < opt) fail("cost " + std::to_string(cost) + " below the length-limited optimum " + std::to_string(opt), A.name, name);
            const double ratio = (double)cost / (double)opt;
            if (ratio > A.worst) { A.worst = ratio; A.worst_name = name; }
        }
        // rarer symbols never get the shorter code
        for (size_t a = 0; a < used_sym.size(); ++a)
            for (size_t b = 0; b < used_sym.size(); ++b)
                if (used[a] < used[b] && len[used_sym[a]] < len[used_sym[b]]) {
                    fail("symbol " + std::to_string(used_sym[a]) + " is rarer than " + std::to_string(used_sym[b]) + " and has the shorter code", A.name, name);
                    a = b = used_sym.size();
                }
    }

    // make_codes against RFC 1951 §3.2.2, and the code prefix-free
    std::memset(code.get(), 0xEE, 2 * (size_t)n);
    make_codes(len.get(), n, code.get());
    int bl_count[16] = {0}, next_code[16] = {0};
    for (int i = 0; i < n; ++i)
        if (len[i]) bl_count[len[i]]++;
    int c = 0;
    for (int bits = 1; bits <= 15; ++bits) {
        c = (c + bl_count[bits - 1]) << 1;
        next_code[bits] = c;
    }
    std::vector<std::pair<uint32_t, int>> msb;  // (code, length), most significant bit first
    for (int i = 0; i < n; ++i) {
        if (!len[i]) {
            if (code[i] != 0) fail("a code for the unused symbol " + std::to_string(i), A.name, name);
            continue;
        }
        const uint32_t want = (uint32_t)next_code[len[i]]++;
        if (want >> len[i]) fail("RFC code does not fit its length: the lengths are over-subscribed", A.name, name);
        if (code[i] != reverse_bits(want, len[i]))
            fail("symbol " + std::to_string(i) + ": code " + std::to_string(code[i]) + ", RFC 1951 (reversed) " +
                 std::to_string(reverse_bits(want, len[i])), A.name, name);
        msb.push_back({reverse_bits(code[i], len[i]), len[i]});
    }
    for (size_t a = 0; a < msb.size(); ++a)
        for (size_t b = 0; b < msb.size(); ++b)
            if (a != b && msb[a].second <= msb[b].second && (msb[b].first >> (msb[b].second - msb[a].second)) == msb[a].first) {
                fail("a code is the prefix of another", A.name, name);
                a = b = msb.size();
            }
}

// ---- the run-length form: decode it the way an inflater does and compare
uint64_t g_rle = 0;
void check_rle(const std::vector<uint8_t>& lit, uint32_t hlit, const std::vector<uint8_t>& dist, uint32_t hdist, const std::string& name) {
    std::unique_ptr<uint8_t[]> ll(new uint8_t[hlit]), dl(new uint8_t[hdist]);
    std::memcpy(ll.get(), lit.data(), hlit);
    std::memcpy(dl.get(), dist.data(), hdist);
    std::unique_ptr<uint16_t[]> rle(new uint16_t[hlit + hdist]);
    const uint32_t nr = rle_lengths(ll.get(), hlit, dl.get(), hdist, rle.get());
    ++g_rle;
    if (nr > hlit + hdist || nr > 320) { fail("more code-length symbols than lengths", "rle", name); return; }
    std::vector<uint8_t> got;
    for (uint32_t k = 0; k < nr; ++k) {
        const uint32_t sym = rle[k] & 0xFFu, ex = rle[k] >> 8;
        if (sym <= 15) {
            if (ex) fail("extra bits on a plain length", "rle", name);
            got.push_back((uint8_t)sym);
        } else if (sym == 16) {
            if (got.empty() || ex > 3) { fail("16 with nothing to repeat, or its count beyond 2 bits", "rle", name); return; }
            got.insert(got.end(), 3 + ex, got.back());
        } else if (sym == 17) {
            if (ex > 7) fail("17: count beyond 3 bits", "rle", name);
            got.insert(got.end(), 3 + ex, 0);
        } else if (sym == 18) {
            if (ex > 127) fail("18: count beyond 7 bits", "rle", name);
            got.insert(got.end(), 11 + ex, 0);
        } else {
            fail("code-length symbol " + std::to_string(sym), "rle", name);
            return;
        }
    }
    std::vector<uint8_t> want(lit.begin(), lit.begin() + hlit);
    want.insert(want.end(), dist.begin(), dist.begin() + hdist);
    if (got != want) fail("the run-length form decodes to other lengths", "rle", name);
}

std::vector<uint32_t> fib(int k) {
    std::vector<uint32_t> v;
    uint32_t a = 1, b = 1;
    for (int i = 0; i < k; ++i) { v.push_back(a); const uint32_t t = a + b; a = b; b = t; }
    return v;
}
uint64_t sum(const std::vector<uint32_t>& v) {
    uint64_t s = 0;
    for (uint32_t x : v) s += x;
    return s;
}

// `vals` on the symbols `where` (or on 0, 1, 2, ... when empty)
std::vector<uint32_t> place(int n, const std::vector<uint32_t>& vals, const std::vector<int>& where = {}) {
    std::vector<uint32_t> f(n, 0);
    for (size_t i = 0; i < vals.size(); ++i) f[where.empty() ? (int)i : where[i]] = vals[i];
    return f;
}

void run_alphabet(Alphabet& A, int n_random, uint64_t seed) {
    const int n = A.n;
    std::mt19937_64 rng(seed * 1000003ull + (uint64_t)n);
    auto below = [&](uint64_t k) { return (uint64_t)(rng() % k); };
    auto unit = [&]() { return (double)(rng() >> 11) * (1.0 / 9007199254740992.0); };
    auto perm = [&](int k) {  // k distinct symbols in random order
        std::vector<int> p(n);
        for (int i = 0; i < n; ++i) p[i] = i;
        for (int i = n - 1; i > 0; --i) std::swap(p[i], p[below((uint64_t)i + 1)]);
        p.resize(k);
        return p;
    };
    auto S = [](const char* a, long long b, const char* c = "", long long d = -1) {
        return std::string(a) + std::to_string(b) + (d >= 0 ? std::string(c) + std::to_string(d) : std::string());
    };

    check(A, place(n, {}), "all zero");
    for (int s : {0, 1, n - 1})
        for (uint32_t v : {1u, 7u, (uint32_t)kMaxSum}) check(A, place(n, {v}, {s}), S("one used symbol ", s, " x ", v));
    for (auto pr : {std::pair<int, int>{0, 1}, {0, n - 1}, {1, 2}, {n - 2, n - 1}, {3, n / 2}})
        for (auto fv : {std::pair<uint32_t, uint32_t>{1, 1}, {1, 65280}, {65280, 1}, {32640, 32641}})
            check(A, place(n, {fv.first, fv.second}, {pr.first, pr.second}), S("two used symbols ", pr.first, ", ", pr.second));
    for (int k = 2; k <= n; ++k)
        for (uint32_t v : {1u, (uint32_t)(kMaxSum / (uint64_t)k)})
            check(A, place(n, std::vector<uint32_t>((size_t)k, v)), S("all equal: ", k, " x ", v));

    // Fibonacci runs: over k symbols an optimal code is k - 1 deep
    for (int k = 2; k <= n && sum(fib(k)) <= kMaxSum; ++k) {
        const std::vector<uint32_t> v = fib(k);
        check(A, place(n, v), S("fibonacci ", k));
        std::vector<uint32_t> r(v.rbegin(), v.rend());
        check(A, place(n, r), S("fibonacci descending ", k));
        for (int rep = 0; rep < 4; ++rep) check(A, place(n, v, perm(k)), S("fibonacci permuted ", k, " #", rep));
        // scaled as far as the sum allows: the same tree without the tie between the first two
        const uint32_t mul = (uint32_t)(kMaxSum / sum(v));
        if (mul > 1) {
            std::vector<uint32_t> s = v;
            for (uint32_t& x : s) x *= mul;
            check(A, place(n, s, perm(k)), S("fibonacci scaled ", k, " x ", mul));
            s[0] -= 1;
            check(A, place(n, s), S("fibonacci scaled, first one less ", k));
        }
        // ties: every number twice, and the run with its small end repeated
        std::vector<uint32_t> twice;
        for (uint32_t x : v) { twice.push_back(x); twice.push_back(x); }
        if ((int)twice.size() <= n && sum(twice) <= kMaxSum) {
            check(A, place(n, twice), S("fibonacci, each twice ", k));
            check(A, place(n, twice, perm((int)twice.size())), S("fibonacci, each twice, permuted ", k));
        }
        for (int ones : {1, 2, 3, 8}) {
            std::vector<uint32_t> t = v;
            t.insert(t.begin(), (size_t)ones, 1u);
            if ((int)t.size() <= n && sum(t) <= kMaxSum) check(A, place(n, t, perm((int)t.size())), S("fibonacci ", k, " and more ones: ", ones));
        }
        // the rest of the alphabet as singletons beside the run
        if (k < n && sum(v) + (uint64_t)(n - k) <= kMaxSum) {
            std::vector<uint32_t> t = v;
            t.resize((size_t)n, 1u);
            check(A, place(n, t), S("fibonacci ", k, " and singletons to ", n));
        }
    }
    // geometric: f_i ~ r^i, floored at 1
    for (double r : {0.3, 0.5, 0.6, 0.618, 0.65, 0.7, 0.8, 0.9, 0.97})
        for (int k : {2, 3, 8, 16, 19, 24, 30, 64, 286}) {
            if (k > n) continue;
            for (uint64_t top : {(uint64_t)40000, (uint64_t)20000, (uint64_t)1000}) {
                std::vector<uint32_t> v;
                double x = (double)top;
                for (int i = 0; i < k; ++i) { v.push_back(x < 1.0 ? 1u : (uint32_t)x); x *= r; }
                if (sum(v) > kMaxSum) continue;
                check(A, place(n, v, perm(k)), S("geometric k ", k, " top ", (long long)top) + " r " + std::to_string(r));
            }
        }
    // one huge symbol and singletons
    for (int j = 1; j < n; ++j) {
        std::vector<uint32_t> v((size_t)j + 1, 1u);
        v[0] = (uint32_t)(kMaxSum - (uint64_t)j);
        check(A, place(n, v), S("one huge and singletons: ", j));
        if (j % 7 == 0) check(A, place(n, v, perm(j + 1)), S("one huge and singletons, permuted: ", j));
    }
    // random supports and skews
    for (int it = 0; it < n_random; ++it) {
        const int m = (int)below((uint64_t)n + 1);
        const double skew = 1.0 + 40.0 * unit() * unit();
        std::vector<double> raw((size_t)m);
        double tot = 0;
        for (double& x : raw) { x = std::pow(unit(), skew); tot += x; }
        const uint64_t budget = (uint64_t)m + below(kMaxSum - (uint64_t)m + 1);
        std::vector<uint32_t> v;
        for (double x : raw) v.push_back(1u + (uint32_t)(tot > 0 ? x / tot * (double)(budget - (uint64_t)m) : 0));
        if (sum(v) > kMaxSum) { std::printf("FAIL: a random vector beyond the sum\n"); ++g_fail; continue; }
        check(A, place(n, v, perm(m)), S("random #", it, " support ", m));
    }
}

void run_rle(int n_random, uint64_t seed) {
    std::mt19937_64 rng(seed + 77);
    auto below = [&](uint64_t k) { return (uint64_t)(rng() % k); };
    std::vector<uint8_t> lit(286, 0), dist(30, 0);
    check_rle(lit, 257, dist, 1, "all zero, smallest");
    check_rle(lit, 286, dist, 30, "all zero, largest");
    for (int v : {1, 8, 15}) {
        check_rle(std::vector<uint8_t>(286, (uint8_t)v), 286, std::vector<uint8_t>(30, (uint8_t)v), 30, "all " + std::to_string(v));
        // every run length of one value and of zeros, ending at and crossing the HLIT / HDIST boundary
        for (int run = 1; run <= 150; ++run)
            for (int end : {257, 258, 260}) {
                if (run >= end) continue;
                for (int zero = 0; zero < 2; ++zero) {
                    std::vector<uint8_t> l(286, (uint8_t)(zero ? 5 : 0)), d(30, (uint8_t)(zero ? 5 : 0));
                    for (int i = end - run; i < end; ++i) (i < 257 ? l[(size_t)i] : d[(size_t)(i - 257)]) = (uint8_t)(zero ? 0 : v);
                    check_rle(l, 257, d, 4, "run " + std::to_string(run) + " ending at " + std::to_string(end));
                }
            }
    }
    for (int it = 0; it < n_random; ++it) {
        const uint32_t hlit = 257 + (uint32_t)below(30), hdist = 1 + (uint32_t)below(30);
        std::vector<uint8_t> l(286, 0), d(30, 0);
        const int kinds = 1 + (int)below(4);
        uint32_t i = 0;
        while (i < hlit + hdist) {  // runs of random lengths out of a few values
            const uint8_t v = below(3) == 0 ? 0 : (uint8_t)(1 + below((uint64_t)kinds) * 3);
            uint32_t run = 1 + (uint32_t)below(below(4) == 0 ? 200 : 9);
            for (; run && i < hlit + hdist; --run, ++i) (i < hlit ? l[i] : d[i - hlit]) = v;
        }
        check_rle(l, hlit, d, hdist, "random #" + std::to_string(it));
    }
}

}  // namespace

int main(int argc, char** argv) {
    const int n_random = argc > 1 ? std::atoi(argv[1]) : 3000;
    const uint64_t seed = argc > 2 ? (uint64_t)std::atoll(argv[2]) : 1;
    Alphabet alphabets[3];
    const char* names[3] = {"literal/length 286/15", "distance 30/15", "code-length 19/7"};
    const int sizes[3] = {286, 30, 19}, limits[3] = {15, 15, 7};
    for (int k = 0; k < 3; ++k) {
        Alphabet& A = alphabets[k];
        A.name = names[k];
        A.n = sizes[k];
        A.maxbits = limits[k];
        run_alphabet(A, n_random, seed);
        std::printf("%s: %llu vectors, limiter needed %llu, optimal depth exactly at the limit %llu, worst cost / optimum %.6f (%s)\n",
                    A.name, (unsigned long long)A.vectors, (unsigned long long)A.limited, (unsigned long long)A.at_limit, A.worst,
                    A.worst_name.c_str());
        if (A.limited == 0 || A.at_limit == 0) {
            std::printf("FAIL [%s]: no vector reached the limiter's edge\n", A.name);
            ++g_fail;
        }
    }
    run_rle(n_random, seed);
    std::printf("run-length form: %llu length sequences\n", (unsigned long long)g_rle);
    double worst = 1.0;
    for (const Alphabet& A : alphabets) worst = std::max(worst, A.worst);
    std::printf("worst cost ratio %.6f\n", worst);
    if (g_fail) {
        std::printf("deflate_huff: %d failures\n", g_fail);
        return 1;
    }
    std::printf("deflate_huff ok\n");
    return 0;
}
