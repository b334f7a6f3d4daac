// ckpt_format.hpp -- the checkpoint blob of the Metropolis-Hastings driver (mcd_mh_save / mcd_mh_load, include/mcmcdate_mvn.h) as plain host
// code: layout constants, the checksum, and the parser behind mcd_ckpt_inspect.  No HIP, no allocation, no handle: ckpt_capi.cpp includes it,
// and so does the stand-alone program tests/cpp/test_ckpt_format.cpp, which runs it under the host sanitizers.
//
// The blob is a sequence of little-endian 8-byte words:
//   fixed header   kCkptFixedWords words (the CKPT_W_* indices below): magic, version, sizes, the configuration in clear and hashed, step
//   section table  n_sections x 4 words: id, offset (bytes from the blob's start), bytes (a multiple of 8), checksum of the section's words
//   header sum     1 word: the checksum of every header word before it (fixed header and table, the sections' checksums included)
//   sections       in the table's order, back to back, the first one at header_bytes
// Checksum of words w[0..n): sum_i mix(w_i XOR (i + 1) 0x9E3779B97F4A7C15) mod 2^64, mix = the splitmix64 finaliser: position-dependent, and
// a wrapping sum, so any order of summation gives the same word (k_checkpoint.hip adds per-wave partial sums with integer atomics).
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../include/mcmcdate_mvn.h"

#ifdef __HIPCC__
#define MCD_CKPT_HD __host__ __device__
#else
#define MCD_CKPT_HD
#endif

namespace mcd {

constexpr uint64_t kCkptMagic = 0x0054504B4344434DULL;   // "MCDCKPT\0"
constexpr uint32_t kCkptVersion = 1;
constexpr int kCkptFixedWords = 16;
constexpr int kCkptMaxSections = MCD_CKPT_MAX_SECTIONS;
constexpr int kCkptMetaWords = 48;

enum {   // fixed header words; "lo | hi": two 32-bit fields in one word
    CKPT_W_MAGIC = 0, CKPT_W_VERSION_HBYTES, CKPT_W_TOTAL, CKPT_W_NSEC_FLAGS, CKPT_W_NODES_PROPS, CKPT_W_BATCH, CKPT_W_DIM_DENSE, CKPT_W_SEED,
    CKPT_W_CHAIN0, CKPT_W_TOPOLOGY, CKPT_W_TABLE, CKPT_W_FINGERPRINT, CKPT_W_STEP
};
enum {   // the words of section MCD_CKPT_SEC_META: what the handle keeps on the host
    CKPT_M_STEP = 0, CKPT_M_N_SAMPLES, CKPT_M_LIK_ONLY, CKPT_M_REC_PERIOD, CKPT_M_REC_ITER, CKPT_M_REC_FETCHED, CKPT_M_MC3_CHAINS, CKPT_M_MC3_TOTAL,
    CKPT_M_MC3_SEED, CKPT_M_MC3_PHASE, CKPT_M_MC3_LADDER /* 16 words */, CKPT_M_HAM = CKPT_M_MC3_LADDER + 16, CKPT_M_HAM_DEPTH, CKPT_M_HAM_SEED,
    CKPT_M_HAM_NEXT, CKPT_M_HAM_COUNTED, CKPT_M_HAM_INV_MASS, CKPT_M_HAM_DIM
};
static_assert(CKPT_M_HAM_DIM < kCkptMetaWords, "");

MCD_CKPT_HD inline uint64_t ckpt_mix(uint64_t z)
{
    z ^= z >> 30;
    z *= 0xBF58476D1CE4E5B9ULL;
    z ^= z >> 27;
    z *= 0x94D049BB133111EBULL;
    z ^= z >> 31;
    return z;
}
inline uint64_t ckpt_term(uint64_t w, uint64_t i) { return ckpt_mix(w ^ ((i + 1) * 0x9E3779B97F4A7C15ULL)); }

// `p` need not be aligned (a caller's buffer): every word is read by memcpy
inline uint64_t ckpt_word(const void* p, uint64_t i)
{
    uint64_t w;
    memcpy(&w, (const unsigned char*)p + 8 * i, 8);
    return w;
}
inline uint64_t ckpt_checksum(const void* p, uint64_t n_words)
{
    uint64_t c = 0;
    for (uint64_t i = 0; i < n_words; ++i) c += ckpt_term(ckpt_word(p, i), i);
    return c;
}

inline uint64_t ckpt_header_words(int n_sections) { return (uint64_t)kCkptFixedWords + 4 * (uint64_t)n_sections + 1; }

// The header of `buf` into *info, every field checked before it is used: 0, or MCD_ERR_INVALID_ARG with the reason in `why`.  payload: also
// recompute every section's checksum (mcd_ckpt_inspect); mcd_mh_load leaves that to the device and checks the header and META here.
inline int ckpt_parse(const void* buf, int64_t len, mcd_ckpt_info_t* info, bool payload, char* why, size_t why_len)
{
    auto bad = [&](const char* fmt, long long a = 0, long long b = 0) {
        snprintf(why, why_len, fmt, a, b);
        return MCD_ERR_INVALID_ARG;
    };
    memset(info, 0, sizeof *info);
    if (!buf || len < 8 * (int64_t)ckpt_header_words(0)) return bad("truncated: %lld bytes cannot hold a checkpoint header", (long long)len);
    if (ckpt_word(buf, CKPT_W_MAGIC) != kCkptMagic) return bad("bad magic: not a checkpoint of mcd_mh_save");
    const uint64_t vh = ckpt_word(buf, CKPT_W_VERSION_HBYTES), nf = ckpt_word(buf, CKPT_W_NSEC_FLAGS);
    const uint32_t version = (uint32_t)vh, hbytes = (uint32_t)(vh >> 32), nsec = (uint32_t)nf;
    if (version != kCkptVersion) return bad("unknown version %lld (this library reads version %lld)", version, kCkptVersion);
    if (nsec < 1 || nsec > (uint32_t)kCkptMaxSections) return bad("the header names %lld sections (1 .. %lld)", nsec, kCkptMaxSections);
    const uint64_t hw = ckpt_header_words((int)nsec);
    if (hbytes != 8 * hw) return bad("the header's size field (%lld) does not fit its %lld sections", hbytes, nsec);
    if ((uint64_t)len < 8 * hw) return bad("truncated: %lld bytes, the header alone has %lld", (long long)len, (long long)(8 * hw));
    const uint64_t total = ckpt_word(buf, CKPT_W_TOTAL);
    if (ckpt_checksum(buf, hw - 1) != ckpt_word(buf, hw - 1)) return bad("the header's checksum does not match its words");
    if (total != (uint64_t)len) return bad("the blob says %lld bytes, the buffer has %lld (truncated?)", (long long)total, (long long)len);
    info->version = (int32_t)version;
    info->header_bytes = (int64_t)hbytes;
    info->total_bytes = (int64_t)total;
    info->n_sections = (int32_t)nsec;
    info->flags = (uint32_t)(nf >> 32);
    const uint64_t np = ckpt_word(buf, CKPT_W_NODES_PROPS), dd = ckpt_word(buf, CKPT_W_DIM_DENSE);
    info->n_nodes = (int32_t)(uint32_t)np;
    info->n_prop = (int32_t)(uint32_t)(np >> 32);
    info->batch = (int64_t)ckpt_word(buf, CKPT_W_BATCH);
    info->dim = (int32_t)(uint32_t)dd;
    info->dense = (int32_t)(uint32_t)(dd >> 32);
    info->seed = ckpt_word(buf, CKPT_W_SEED);
    info->chain0 = (int64_t)ckpt_word(buf, CKPT_W_CHAIN0);
    info->topology = ckpt_word(buf, CKPT_W_TOPOLOGY);
    info->table = ckpt_word(buf, CKPT_W_TABLE);
    info->fingerprint = ckpt_word(buf, CKPT_W_FINGERPRINT);
    info->step = ckpt_word(buf, CKPT_W_STEP);
    uint64_t at = 8 * hw;                                  // sections lie back to back behind the header
    for (uint32_t s = 0; s < nsec; ++s) {
        const uint64_t id = ckpt_word(buf, kCkptFixedWords + 4 * s), off = ckpt_word(buf, kCkptFixedWords + 4 * s + 1),
                       bytes = ckpt_word(buf, kCkptFixedWords + 4 * s + 2);
        if (off != at || bytes % 8 != 0 || bytes > total - at) return bad("section %lld of the table leaves the blob or the sections' order", s);
        at += bytes;
        info->section_id[s] = (int32_t)(uint32_t)id;
        info->section_offset[s] = (int64_t)off;
        info->section_bytes[s] = (int64_t)bytes;
        info->section_checksum[s] = ckpt_word(buf, kCkptFixedWords + 4 * s + 3);
    }
    if (at != total) return bad("the sections end at byte %lld, the blob at %lld", (long long)at, (long long)total);
    if (info->section_id[0] != MCD_CKPT_SEC_META || info->section_bytes[0] != 8 * kCkptMetaWords)
        return bad("the first section is not the handle's counters (%lld bytes)", (long long)info->section_bytes[0]);
    for (uint32_t s = 0; s < nsec; ++s) {
        if (!payload && s > 0) break;
        if (ckpt_checksum((const unsigned char*)buf + info->section_offset[s], (uint64_t)info->section_bytes[s] / 8) != info->section_checksum[s])
            return bad("section %lld (id %lld): its checksum does not match its bytes", s, info->section_id[s]);
    }
    return MCD_OK;
}

}  // namespace mcd
