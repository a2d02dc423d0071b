// kvarq_amd/csrc/kvq_dup_hash.h -- the hash of a record's duplication key (include/kvarq_hip.h): ONE function for
// the kernel (kernels_reads.hip), the CPU twin (kvq_reads_host) and the table's settle kernels.  Order-free over the key's eight
// words, so that on the device every lane mixes the words it holds and the wave XORs the parts.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define KVQ_HD __host__ __device__ __forceinline__
#else
#define KVQ_HD static inline
#endif

#define KVQ_DUP_KEY_BYTES 64
#define KVQ_DUP_G 0x9E3779B97F4A7C15ull

// m of the definition (the finalizer of splitmix64)
KVQ_HD uint64_t kvq_dup_mix(uint64_t x)
{
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}
// the part of word i (0 .. 7) of the zero-padded key
KVQ_HD uint64_t kvq_dup_word(uint64_t w, uint32_t i) { return kvq_dup_mix(w + (uint64_t)(i + 1u) * KVQ_DUP_G); }
// the hash from the key's length n (1 .. 64) and the XOR of its eight parts; never 0 (0 marks an empty slot of the table)
KVQ_HD uint64_t kvq_dup_close(uint32_t n, uint64_t parts)
{
    const uint64_t h = kvq_dup_mix(kvq_dup_mix((uint64_t)n + KVQ_DUP_G) ^ parts);
    return h ? h : 1ull;
}
// the hash of the key of a bases line of L bytes (its trailing '\r' already taken off; L >= 1): its first min(L, 64) bytes
KVQ_HD uint64_t kvq_dup_hash(const uint8_t *line, uint64_t L)
{
    const uint32_t n = L < KVQ_DUP_KEY_BYTES ? (uint32_t)L : (uint32_t)KVQ_DUP_KEY_BYTES;
    uint64_t parts = 0;
    for (uint32_t i = 0; i < 8u; i++) {
        uint64_t w = 0;
        for (uint32_t j = 0; j < 8u; j++) if (8u * i + j < n) w |= (uint64_t)line[8u * i + j] << (8u * j);
        parts ^= kvq_dup_word(w, i);
    }
    return kvq_dup_close(n, parts);
}
// key h is tracked at level s when its s low bits are zero
KVQ_HD bool kvq_dup_tracked(uint64_t h, uint32_t s) { return s >= 64u ? h == 0ull : (h & ((1ull << s) - 1ull)) == 0ull; }
// the count bin (0 .. 15) of a key with c >= 1 copies: lower bounds 1 .. 10, 50, 100, 500, 1000, 5000, 10000
KVQ_HD uint32_t kvq_dup_bin(uint64_t c)
{
    return c < 10ull ? (uint32_t)c - 1u : c < 50ull ? 9u : c < 100ull ? 10u : c < 500ull ? 11u : c < 1000ull ? 12u : c < 5000ull ? 13u : c < 10000ull ? 14u : 15u;
}
