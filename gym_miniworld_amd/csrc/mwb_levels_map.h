// mwb_levels_map.h - level sets: which level an env plays next, the level's seed, and the MT19937 row that seed stands for.
//
// Plain C++ without any HIP type, so that the same functions run in the kernels (mwb_levels.hip), in the host API (mwb_seed and
// mwb_seed_key of mwb_api.hip call them: there is no second copy) and in a host program (tests/test_levels_host.py builds one
// around this header).
//
// The reference: a level is what Procgen calls one (`num_levels` / `start_level`: a finite, named set of worlds), and an episode in
// level seed s is the first episode of a reference env after `env.seed(s); env.reset()` - gym<=0.21's seeding.np_random(s) hashes
// the decimal string of s with SHA-512, keeps the first 8 bytes as little-endian 32-bit limbs (the high limb dropped when it is
// zero) and hands them to RandomState.seed(list) = MT19937 init_by_array.
//
// A set has L levels, 1 <= L <= 2^31 - 1; level i has the seed seeds[i] where a table was given, start_level + i (uint64
// arithmetic) otherwise.  The level of an env's n-th assignment depends only on (g, n, request) - g the env's global index
// env_offset + e, n its episode_no - never on the order of the regenerated-env list:
//
//   SEQUENTIAL   i = (g + n * stride) mod L                 with L = q * stride, q episodes per env visit every level once
//   UNIFORM      a = mix(sampler_seed + GOLD * (g + 1)), h = mix(a + GOLD * (n + 1)), i = (h * L) >> 64   (mix = splitmix64's)
//   TABLE        the request next_level[e] where 0 <= request < L, otherwise the UNIFORM level; a request other than -1 that is
//                out of range is counted as rejected, and no address is formed from it
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MWB_LEVELS_HD __host__ __device__
#define MWB_LEVELS_UNROLL _Pragma("unroll")
#define MWB_LEVELS_NOUNROLL _Pragma("nounroll")
#else
#define MWB_LEVELS_HD
#define MWB_LEVELS_UNROLL
#define MWB_LEVELS_NOUNROLL
#endif

#define MWB_LEVELS_MODE_SEQUENTIAL 0
#define MWB_LEVELS_MODE_UNIFORM 1
#define MWB_LEVELS_MODE_TABLE 2
#define MWB_LEVELS_MAX 2147483647LL               // levels of a set
#define MWB_LEVELS_MAX_TABLE (1LL << 24)          // ... of one with an explicit seed table
#define MWB_LEVELS_MAX_TALLY (1LL << 22)          // ... of one with tallies
#define MWB_LEVELS_GOLD 0x9E3779B97F4A7C15ULL

// ------------------------------------------------------------------------------------------------ the rules
MWB_LEVELS_HD static inline uint64_t mwb_levels_mix(uint64_t z) {
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ULL;
    z ^= z >> 27; z *= 0x94D049BB133111EBULL;
    z ^= z >> 31;
    return z;
}

// high word of the 128-bit product, from 32-bit halves (the same arithmetic on the host and in a kernel)
MWB_LEVELS_HD static inline uint64_t mwb_levels_mulhi(uint64_t a, uint64_t b) {
    const uint64_t a0 = (uint32_t)a, a1 = a >> 32, b0 = (uint32_t)b, b1 = b >> 32;
    const uint64_t p00 = a0 * b0, p01 = a0 * b1, p10 = a1 * b0, p11 = a1 * b1;
    const uint64_t mid = (p00 >> 32) + (uint32_t)p01 + (uint32_t)p10;
    return p11 + (p01 >> 32) + (p10 >> 32) + (mid >> 32);
}

// x mod L for L < 2^31 without a 64-bit division (in a kernel that is a long subroutine with branches of its own): the high word by
// a 32-bit division, then the low word bit by bit - the remainder stays below L, so twice it plus one bit fits 32 bits
MWB_LEVELS_HD static inline uint32_t mwb_levels_mod(uint64_t x, uint32_t L) {
    uint32_t r = (uint32_t)(x >> 32) % L;
    const uint32_t lo = (uint32_t)x;
    for (int b = 31; b >= 0; b--) {
        r = (r << 1) | ((lo >> b) & 1u);
        r -= r >= L ? L : 0u;
    }
    return r;
}

// (g + n * stride) mod L, evaluated without overflow as ((g % L) + ((n % L) * (stride % L)) % L) % L
MWB_LEVELS_HD static inline int32_t mwb_levels_sequential(uint64_t g, uint64_t n, uint64_t stride, uint64_t L) {
    const uint32_t l = (uint32_t)L;
    const uint32_t a = mwb_levels_mod(g, l), b = mwb_levels_mod((uint64_t)mwb_levels_mod(n, l) * mwb_levels_mod(stride, l), l);   // the product is < 2^62
    const uint32_t sum = a + b;   // < 2^32
    return (int32_t)(sum >= l ? sum - l : sum);
}

MWB_LEVELS_HD static inline int32_t mwb_levels_uniform(uint64_t sampler_seed, uint64_t g, uint64_t n, uint64_t L) {
    const uint64_t a = mwb_levels_mix(sampler_seed + MWB_LEVELS_GOLD * (g + 1));
    const uint64_t h = mwb_levels_mix(a + MWB_LEVELS_GOLD * (n + 1));
    return (int32_t)mwb_levels_mulhi(h, L);
}

// the level of assignment n of env g.  request: next_level[e] (only read in TABLE mode); *rejected = 1 where it was out of range
MWB_LEVELS_HD static inline int32_t mwb_levels_choose(int mode, uint64_t g, uint64_t n, uint64_t L, uint64_t stride, uint64_t sampler_seed,
                                                      int32_t request, int *rejected) {
    *rejected = 0;
    if (mode == MWB_LEVELS_MODE_SEQUENTIAL) return mwb_levels_sequential(g, n, stride, L);
    if (mode == MWB_LEVELS_MODE_TABLE) {
        if (request >= 0 && (uint64_t)request < L) return request;
        *rejected = request != -1;
    }
    return mwb_levels_uniform(sampler_seed, g, n, L);
}

// the seed of level i (0 <= i < L); table: the L seeds, or null
MWB_LEVELS_HD static inline uint64_t mwb_levels_seed_of(int32_t i, uint64_t start_level, const uint64_t *table) {
    return table ? table[i] : start_level + (uint64_t)i;
}

// ------------------------------------------------------------------------------------------------ SHA-512 of a decimal uint64
MWB_LEVELS_HD static inline uint64_t mwb_levels_rotr(uint64_t x, int n) { return (x >> n) | (x << (64 - n)); }

// byte b at position k (0 .. 23) of a big-endian message held in three words: selects, no indexed array
MWB_LEVELS_HD static inline void mwb_levels_put(uint64_t &w0, uint64_t &w1, uint64_t &w2, int k, uint64_t b) {
    const uint64_t v = b << (56 - 8 * (k & 7));
    const int word = k >> 3;
    w0 |= word == 0 ? v : 0; w1 |= word == 1 ? v : 0; w2 |= word == 2 ? v : 0;
}

// digest[8] = SHA-512(str(seed)) as eight big-endian words.  The message is at most 20 digits: one block, whose words 3 .. 14 are
// zero; the schedule is a rolling window of 16 words.
MWB_LEVELS_HD static inline void mwb_levels_sha512_decimal(uint64_t seed, uint64_t digest[8]) {
    const uint64_t K[80] = {
        0x428a2f98d728ae22ULL, 0x7137449123ef65cdULL, 0xb5c0fbcfec4d3b2fULL, 0xe9b5dba58189dbbcULL, 0x3956c25bf348b538ULL,
        0x59f111f1b605d019ULL, 0x923f82a4af194f9bULL, 0xab1c5ed5da6d8118ULL, 0xd807aa98a3030242ULL, 0x12835b0145706fbeULL,
        0x243185be4ee4b28cULL, 0x550c7dc3d5ffb4e2ULL, 0x72be5d74f27b896fULL, 0x80deb1fe3b1696b1ULL, 0x9bdc06a725c71235ULL,
        0xc19bf174cf692694ULL, 0xe49b69c19ef14ad2ULL, 0xefbe4786384f25e3ULL, 0x0fc19dc68b8cd5b5ULL, 0x240ca1cc77ac9c65ULL,
        0x2de92c6f592b0275ULL, 0x4a7484aa6ea6e483ULL, 0x5cb0a9dcbd41fbd4ULL, 0x76f988da831153b5ULL, 0x983e5152ee66dfabULL,
        0xa831c66d2db43210ULL, 0xb00327c898fb213fULL, 0xbf597fc7beef0ee4ULL, 0xc6e00bf33da88fc2ULL, 0xd5a79147930aa725ULL,
        0x06ca6351e003826fULL, 0x142929670a0e6e70ULL, 0x27b70a8546d22ffcULL, 0x2e1b21385c26c926ULL, 0x4d2c6dfc5ac42aedULL,
        0x53380d139d95b3dfULL, 0x650a73548baf63deULL, 0x766a0abb3c77b2a8ULL, 0x81c2c92e47edaee6ULL, 0x92722c851482353bULL,
        0xa2bfe8a14cf10364ULL, 0xa81a664bbc423001ULL, 0xc24b8b70d0f89791ULL, 0xc76c51a30654be30ULL, 0xd192e819d6ef5218ULL,
        0xd69906245565a910ULL, 0xf40e35855771202aULL, 0x106aa07032bbd1b8ULL, 0x19a4c116b8d2d0c8ULL, 0x1e376c085141ab53ULL,
        0x2748774cdf8eeb99ULL, 0x34b0bcb5e19b48a8ULL, 0x391c0cb3c5c95a63ULL, 0x4ed8aa4ae3418acbULL, 0x5b9cca4f7763e373ULL,
        0x682e6ff3d6b2b8a3ULL, 0x748f82ee5defb2fcULL, 0x78a5636f43172f60ULL, 0x84c87814a1f0ab72ULL, 0x8cc702081a6439ecULL,
        0x90befffa23631e28ULL, 0xa4506cebde82bde9ULL, 0xbef9a3f7b2c67915ULL, 0xc67178f2e372532bULL, 0xca273eceea26619cULL,
        0xd186b8c721c0c207ULL, 0xeada7dd6cde0eb1eULL, 0xf57d4f7fee6ed178ULL, 0x06f067aa72176fbaULL, 0x0a637dc5a2c898a6ULL,
        0x113f9804bef90daeULL, 0x1b710b35131c471bULL, 0x28db77f523047d84ULL, 0x32caab7b40c72493ULL, 0x3c9ebe0a15c9bebcULL,
        0x431d67c49c100d4cULL, 0x4cc5d4becb3e42b6ULL, 0x597f299cfc657e2aULL, 0x5fcb6fab3ad6faecULL, 0x6c44198c4a475817ULL};
    // the decimal digits, most significant first, then the 0x80 that ends the message
    int len = 1;
    for (uint64_t p = 10; len < 20 && seed >= p; p *= 10) len++;   // (10^19 < 2^64 <= 10^20: p never overflows before the loop ends)
    uint64_t w0 = 0, w1 = 0, w2 = 0, rest = seed;
    mwb_levels_put(w0, w1, w2, len, 0x80);
MWB_LEVELS_NOUNROLL
    for (int j = 0; j < len; j++) {   // (rolled: unrolled, every step's division becomes constants of its own)
        mwb_levels_put(w0, w1, w2, len - 1 - j, 0x30 + rest % 10);
        rest /= 10;
    }
    uint64_t w[16] = {w0, w1, w2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, (uint64_t)len * 8};
    const uint64_t H0[8] = {0x6a09e667f3bcc908ULL, 0xbb67ae8584caa73bULL, 0x3c6ef372fe94f82bULL, 0xa54ff53a5f1d36f1ULL,
                            0x510e527fade682d1ULL, 0x9b05688c2b3e6c1fULL, 0x1f83d9abfb41bd6bULL, 0x5be0cd19137e2179ULL};
    uint64_t a = H0[0], b = H0[1], c = H0[2], d = H0[3], e = H0[4], f = H0[5], g = H0[6], h = H0[7];
MWB_LEVELS_NOUNROLL
    for (int r = 0; r < 80; r += 16) {   // five rounds of sixteen: inside one the window's indices are constants
MWB_LEVELS_UNROLL
        for (int u = 0; u < 16; u++) {
            if (r) {
                const uint64_t x = w[(u + 1) & 15], y = w[(u + 14) & 15];
                const uint64_t s0 = mwb_levels_rotr(x, 1) ^ mwb_levels_rotr(x, 8) ^ (x >> 7);
                const uint64_t s1 = mwb_levels_rotr(y, 19) ^ mwb_levels_rotr(y, 61) ^ (y >> 6);
                w[u] = w[u] + s0 + w[(u + 9) & 15] + s1;
            }
            const uint64_t S1 = mwb_levels_rotr(e, 14) ^ mwb_levels_rotr(e, 18) ^ mwb_levels_rotr(e, 41);
            const uint64_t ch = (e & f) ^ (~e & g);
            const uint64_t t1 = h + S1 + ch + K[r + u] + w[u];
            const uint64_t S0 = mwb_levels_rotr(a, 28) ^ mwb_levels_rotr(a, 34) ^ mwb_levels_rotr(a, 39);
            const uint64_t maj = (a & b) ^ (a & c) ^ (b & c);
            const uint64_t t2 = S0 + maj;
            h = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
        }
    }
    digest[0] = H0[0] + a; digest[1] = H0[1] + b; digest[2] = H0[2] + c; digest[3] = H0[3] + d;
    digest[4] = H0[4] + e; digest[5] = H0[5] + f; digest[6] = H0[6] + g; digest[7] = H0[7] + h;
}

MWB_LEVELS_HD static inline uint32_t mwb_levels_bswap32(uint32_t x) {
    return (x >> 24) | ((x >> 8) & 0xFF00u) | ((x << 8) & 0xFF0000u) | (x << 24);
}

// seed (already reduced mod 2^64 by the uint64 type) -> MT19937 init_by_array key; returns the key's length: the first 8 digest
// bytes as little-endian limbs, and _int_list_from_bigint drops the high limb when it is zero ([0] for 0)
MWB_LEVELS_HD static inline int mwb_levels_seed_key(uint64_t seed, uint32_t key[2]) {
    uint64_t dig[8];
    mwb_levels_sha512_decimal(seed, dig);
    key[0] = mwb_levels_bswap32((uint32_t)(dig[0] >> 32));
    key[1] = mwb_levels_bswap32((uint32_t)dig[0]);
    return key[1] != 0 ? 2 : 1;
}

// ------------------------------------------------------------------------------------------------ MT19937 init_by_array
// the constant first loop, init_genrand(19650218): 624 words, the same for every key
MWB_LEVELS_HD static inline void mwb_levels_mt_base(uint32_t base[624]) {
    base[0] = 19650218u;
    for (int i = 1; i < 624; i++) base[i] = 1812433253u * (base[i - 1] ^ (base[i - 1] >> 30)) + (uint32_t)i;
}

#define MWB_LEVELS_AHEAD 4   // the third loop reads the row this many words ahead of the chain (622 = 4 * 155 + 2)
static_assert((624 - 2 - 2) % MWB_LEVELS_AHEAD == 0, "mwb_levels_init_by_array: groups of MWB_LEVELS_AHEAD words, then two");

// numpy RandomState.seed(list) == init_by_array, for a key of length 1 or 2 (a select, not a branch), into a row reached through
// `row`: uint32_t row.get(int i) and void row.set(int i, uint32_t v), i = 0 .. 624 (word 624 is the position).  The chain lives in
// `prev`; every new word is stored at once, and the third loop - which needs the second loop's words again - reads them
// MWB_LEVELS_AHEAD iterations before the chain gets there.  base: mwb_levels_mt_base's words.
template <typename Row>
MWB_LEVELS_HD static inline void mwb_levels_init_by_array(Row &row, const uint32_t *base, uint32_t key0, uint32_t key1, int key_length) {
    const uint32_t odd = key_length == 2 ? key1 + 1u : key0;   // init_key[j] + j at j = 1 (length 1: j stays 0)
    uint32_t prev = base[0];
    // second loop: 624 iterations, i = 1 .. 623, then mt[0] = mt[623] and once more at i = 1
    for (int i = 1; i < 624; i++) {
        prev = (base[i] ^ ((prev ^ (prev >> 30)) * 1664525u)) + (((i - 1) & 1) ? odd : key0);
        row.set(i, prev);
    }
    uint32_t one = row.get(1);
    one = (one ^ ((prev ^ (prev >> 30)) * 1664525u)) + odd;   // iteration 623: j = 623 mod key_length
    prev = one;
    // third loop: 623 iterations, i = 2 .. 623, then mt[0] = mt[623] and once more at i = 1
    uint32_t q[MWB_LEVELS_AHEAD];
MWB_LEVELS_UNROLL
    for (int u = 0; u < MWB_LEVELS_AHEAD; u++) q[u] = row.get(2 + u);
    int i = 2;
    for (; i + 2 * MWB_LEVELS_AHEAD <= 624; i += MWB_LEVELS_AHEAD) {   // i = 2 .. 614: the words read ahead end at 621
MWB_LEVELS_UNROLL
        for (int u = 0; u < MWB_LEVELS_AHEAD; u++) {
            const uint32_t cur = q[u];
            q[u] = row.get(i + u + MWB_LEVELS_AHEAD);
            prev = (cur ^ ((prev ^ (prev >> 30)) * 1566083941u)) - (uint32_t)(i + u);
            row.set(i + u, prev);
        }
    }
    const uint32_t last[2] = {row.get(622), row.get(623)};   // i = 618 now: q holds 618 .. 621
MWB_LEVELS_UNROLL
    for (int u = 0; u < MWB_LEVELS_AHEAD + 2; u++) {
        const uint32_t cur = u < MWB_LEVELS_AHEAD ? q[u < MWB_LEVELS_AHEAD ? u : 0] : last[u < MWB_LEVELS_AHEAD ? 0 : u - MWB_LEVELS_AHEAD];
        prev = (cur ^ ((prev ^ (prev >> 30)) * 1566083941u)) - (uint32_t)(i + u);
        row.set(i + u, prev);
    }
    one = (one ^ ((prev ^ (prev >> 30)) * 1566083941u)) - 1u;
    row.set(1, one);
    row.set(0, 0x80000000u);
    row.set(624, 624u);   // position: the first draw regenerates the state
}

// a row in plain memory (the host; a test)
struct MwbLevelsPlainRow {
    uint32_t *mt;
    MWB_LEVELS_HD uint32_t get(int i) const { return mt[i]; }
    MWB_LEVELS_HD void set(int i, uint32_t v) { mt[i] = v; }
};
