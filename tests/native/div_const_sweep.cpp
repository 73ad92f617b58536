// Sweeps div_const (csrc/stencil_math.hpp) against true division over every binade of float and
// double, from the smallest subnormal to the largest finite value, and prints what it finds; the
// judging is done by tests/test_div_const_cpu.py. Build: -O2 -std=c++17 -ffp-contract=off -pthread.
//
//   H <type> <h> <b as %a> <y = RN(1/b) as %a>
//   B <type> <h> <e> <n> <mismatch> <nonfinite> <maxulp>     numerators +-[2^e, 2^(e+1))
//   S <type> <h> <name> <div_const result> <true quotient>   special numerators, as text
//
// type = f32 / f64, h = index of the divisor. mismatch counts the numerators whose result differs
// from a / b in any bit (or in being NaN), nonfinite those of them where either side is NaN or inf
// (div_const's NaN for a finite or an overflowing quotient), maxulp the largest distance in units in
// the last place among the others.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <string>
#include <thread>
#include <vector>

#include "stencil_math.hpp"

namespace {

// the divisors: the h^2 of the GPU tests, and one above 1
const double kH2[] = {0.011, 0.013, 0.017, 2.75};
constexpr int kNH = int(sizeof(kH2) / sizeof(kH2[0]));

struct Rng {  // xorshift64*
    uint64_t s;
    uint64_t next() {
        s ^= s >> 12;
        s ^= s << 25;
        s ^= s >> 27;
        return s * 0x2545F4914F6CDD1DULL;
    }
};

template <class T>
struct Bits;
template <>
struct Bits<float> {
    using I = int32_t;
    using U = uint32_t;
    static constexpr int mant = 23;
    static const char* name() { return "f32"; }
};
template <>
struct Bits<double> {
    using I = int64_t;
    using U = uint64_t;
    static constexpr int mant = 52;
    static const char* name() { return "f64"; }
};

template <class T>
typename Bits<T>::U bits(T x) {
    typename Bits<T>::U u;
    std::memcpy(&u, &x, sizeof u);
    return u;
}
template <class T>
T from_bits(typename Bits<T>::U u) {
    T x;
    std::memcpy(&x, &u, sizeof x);
    return x;
}
// sign-magnitude to an integer that counts representable values monotonically (-0 and +0 coincide)
template <class T>
int64_t ordered(T x) {
    using U = typename Bits<T>::U;
    const U u = bits(x), sign = U(1) << (sizeof(U) * 8 - 1);
    const int64_t mag = int64_t(u & (sign - 1));
    return (u & sign) ? -mag : mag;
}
template <class T>
uint64_t ulp_distance(T a, T b) {
    const int64_t x = ordered(a), y = ordered(b);
    return x > y ? uint64_t(x) - uint64_t(y) : uint64_t(y) - uint64_t(x);
}

// printf into a string: the divisors are swept by one thread each and printed in order
template <class... A>
void put(std::string& out, const char* fmt, A... a) {
    char buf[256];
    std::snprintf(buf, sizeof buf, fmt, a...);
    out += buf;
}

template <class T>
void sweep(long n, int h, std::string& out) {
    using U = typename Bits<T>::U;
    constexpr int mant = Bits<T>::mant;
    const int emin = std::numeric_limits<T>::min_exponent - 1;  // -126 / -1022
    const int emax = std::numeric_limits<T>::max_exponent - 1;  // 127 / 1023
    const char* tn = Bits<T>::name();
    volatile T one = T(1);  // keeps 1/b a run-time division
    const T b = T(kH2[h]);
    const T y = one / b;
    put(out, "H %s %d %a %a\n", tn, h, double(b), double(y));
    Rng rng{0x9E3779B97F4A7C15ULL + uint64_t(h) * 1000003u + sizeof(T)};
    for (int e = emin - mant; e <= emax; ++e) {
        // bit patterns of [2^e, 2^(e+1)): subnormals have e - (emin - mant) free low bits
        const int free_bits = e < emin ? e - (emin - mant) : mant;
        const U base = e < emin ? U(1) << free_bits : U(e - emin + 1) << mant;
        const U mask = (U(1) << free_bits) - 1;
        long mism = 0, nonfin = 0;
        uint64_t maxulp = 0;
        for (long s = 0; s < n; ++s) {
            const uint64_t r = rng.next();
            T a = from_bits<T>(base | (U(r >> 8) & mask));
            if (r & 1) a = -a;
            const T got = wave3d::div_const(a, b, y);
            const T want = a / b;
            const bool gn = got != got, wn = want != want;
            if (gn == wn && (gn || bits(got) == bits(want))) continue;
            ++mism;
            if (gn || wn || std::isinf(got) || std::isinf(want)) {
                ++nonfin;
                continue;
            }
            const uint64_t d = ulp_distance(got, want);
            if (d > maxulp) maxulp = d;
        }
        put(out, "B %s %d %d %ld %ld %ld %llu\n", tn, h, e, n, mism, nonfin, (unsigned long long)maxulp);
    }
    const T inf = std::numeric_limits<T>::infinity(), nan = std::numeric_limits<T>::quiet_NaN();
    const struct {
        const char* name;
        T a;
    } sp[] = {{"+0", T(0)}, {"-0", -T(0)}, {"+inf", inf}, {"-inf", -inf}, {"nan", nan}};
    for (const auto& v : sp) {
        volatile T a = v.a;
        const T got = wave3d::div_const(T(a), b, y);
        const T want = T(a) / b;
        put(out, "S %s %d %s %s%g %s%g\n", tn, h, v.name, std::signbit(got) && got == got ? "-" : "+",
            std::fabs(double(got)), std::signbit(want) && want == want ? "-" : "+", std::fabs(double(want)));
    }
}

}  // namespace

int main(int argc, char** argv) {
    const long n = argc > 1 ? std::atol(argv[1]) : 100000;
    if (n <= 0) return 2;
    std::string out[2 * kNH];
    std::vector<std::thread> pool;
    for (int h = 0; h < kNH; ++h) {
        pool.emplace_back(sweep<float>, n, h, std::ref(out[h]));
        pool.emplace_back(sweep<double>, n, h, std::ref(out[kNH + h]));
    }
    for (auto& t : pool) t.join();
    for (const auto& o : out) std::fputs(o.c_str(), stdout);
    return 0;
}
