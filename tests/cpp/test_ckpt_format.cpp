// Stand-alone host check of csrc/ckpt_format.hpp (no GPU, no library): the parser behind mcd_ckpt_inspect and mcd_mh_load over a valid blob,
// over EVERY prefix of it and over every single-byte corruption of its header (each byte with one bit flipped, inverted, set to 0 and to
// 0xFF).  Every buffer is a heap block of exactly the length handed to the parser, so a read past it is a sanitizer report.  Every
// corrupted header must be refused (the header's checksum covers all of its words); a damaged section is found by the payload pass.
// Meant for a sanitizer build:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/cpp/test_ckpt_format.cpp -o test_ckpt_format
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../mcmc-date_amd/csrc/ckpt_format.hpp"

using namespace mcd;

static std::vector<uint64_t> valid_blob()
{
    const uint32_t ids[4] = {MCD_CKPT_SEC_META, MCD_CKPT_SEC_SC, MCD_CKPT_SEC_HEIGHTS, MCD_CKPT_SEC_ACCEPTED};
    const uint64_t words[4] = {(uint64_t)kCkptMetaWords, 15, 21, 0};      // (an empty section is legal)
    const uint64_t hw = ckpt_header_words(4);
    uint64_t total = hw;
    for (uint64_t w : words) total += w;
    std::vector<uint64_t> b(total, 0);
    for (uint64_t i = hw; i < total; ++i) b[i] = ckpt_mix(i * 77 + 1);
    b[CKPT_W_MAGIC] = kCkptMagic;
    b[CKPT_W_VERSION_HBYTES] = (uint64_t)kCkptVersion | (8 * hw) << 32;
    b[CKPT_W_TOTAL] = 8 * total;
    b[CKPT_W_NSEC_FLAGS] = 4 | (uint64_t)MCD_CKPT_FLAG_DENSE << 32;
    b[CKPT_W_NODES_PROPS] = 7 | (uint64_t)19 << 32;
    b[CKPT_W_BATCH] = 3;
    b[CKPT_W_DIM_DENSE] = 5 | (uint64_t)1 << 32;
    b[CKPT_W_SEED] = 0xFEDCBA9876543210ULL;
    b[CKPT_W_STEP] = 12345;
    uint64_t at = hw;
    for (int s = 0; s < 4; ++s) {
        uint64_t* row = b.data() + kCkptFixedWords + 4 * s;
        row[0] = ids[s];
        row[1] = 8 * at;
        row[2] = 8 * words[s];
        row[3] = ckpt_checksum(b.data() + at, words[s]);
        at += words[s];
    }
    b[hw - 1] = ckpt_checksum(b.data(), hw - 1);
    return b;
}

// the parser on a heap copy of exactly `len` bytes; returns its code
static int parse_copy(const unsigned char* src, size_t len, mcd_ckpt_info_t* info, bool payload)
{
    std::unique_ptr<unsigned char[]> p(new unsigned char[len ? len : 1]);
    if (len) memcpy(p.get(), src, len);
    char why[256] = "";
    const int rc = ckpt_parse(len ? p.get() : nullptr, (int64_t)len, info, payload, why, sizeof why);
    if (rc != MCD_OK && why[0] == 0) {
        fprintf(stderr, "a refusal without a reason (len %zu)\n", len);
        exit(1);
    }
    return rc;
}

int main()
{
    const std::vector<uint64_t> blob = valid_blob();
    const unsigned char* bytes = (const unsigned char*)blob.data();
    const size_t len = 8 * blob.size();
    mcd_ckpt_info_t info;
    long checks = 0;
    if (parse_copy(bytes, len, &info, true) != MCD_OK || info.n_sections != 4 || info.batch != 3 || info.n_nodes != 7 || info.n_prop != 19 ||
        info.seed != 0xFEDCBA9876543210ULL || info.section_bytes[3] != 0 || info.total_bytes != (int64_t)len) {
        fprintf(stderr, "the valid blob was not parsed as built\n");
        return 1;
    }
    {   // an unaligned copy: a caller's buffer need not be aligned
        std::unique_ptr<unsigned char[]> p(new unsigned char[len + 1]);
        memcpy(p.get() + 1, bytes, len);
        char why[256];
        if (ckpt_parse(p.get() + 1, (int64_t)len, &info, true, why, sizeof why) != MCD_OK) return 1;
    }
    for (size_t n = 0; n < len; ++n, ++checks)                       // every prefix is refused
        if (parse_copy(bytes, n, &info, n % 2 == 0) == MCD_OK) {
            fprintf(stderr, "a prefix of %zu bytes was accepted\n", n);
            return 1;
        }
    const size_t header = (size_t)(8 * ckpt_header_words(4));
    std::vector<unsigned char> x(bytes, bytes + len);
    for (size_t i = 0; i < header; ++i) {
        const unsigned char was = x[i];
        const unsigned char tries[4] = {(unsigned char)(was ^ (1u << (i % 8))), (unsigned char)~was, 0, 0xFF};
        for (unsigned char t : tries) {
            if (t == was) continue;
            x[i] = t;
            ++checks;
            if (parse_copy(x.data(), len, &info, true) == MCD_OK) {
                fprintf(stderr, "header byte %zu = 0x%02x was accepted\n", i, t);
                return 1;
            }
        }
        x[i] = was;
    }
    for (size_t i = header; i < len; ++i) {                          // ... and a damaged section by the payload pass alone
        x[i] ^= 0x04;
        ++checks;
        const bool meta = i < header + 8 * (size_t)kCkptMetaWords;
        if (parse_copy(x.data(), len, &info, true) == MCD_OK || (parse_copy(x.data(), len, &info, false) == MCD_OK) == meta) {
            fprintf(stderr, "section byte %zu: damage not found where it should be\n", i);
            return 1;
        }
        x[i] ^= 0x04;
    }
    printf("ckpt_format: %ld damaged or truncated blobs refused, the valid one parsed\n", checks);
    return 0;
}
