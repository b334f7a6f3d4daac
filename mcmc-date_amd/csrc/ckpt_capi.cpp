// ckpt_capi.cpp -- C ABI of checkpoint and continue (include/mcmcdate_mvn.h: mcd_mh_save_size, mcd_mh_save, mcd_mh_load, mcd_ckpt_inspect,
// mcd_ckpt_checksum; the reference's `Settings ... Save` / `continue`, app/Main.hs:494-509, and `--init-from-save`, :424-440).  A save is one
// launch (k_checkpoint.hip: k_ckpt_pack) and one copy to the host; a load one copy to the device, k_ckpt_verify, the host's comparison of the
// checksums, k_ckpt_unpack.  Everything is enqueued on the sampler's stream, which is waited for once at the end (a load also waits for the
// verified checksums).  The blob's format and its host parser: ckpt_format.hpp; the handle's side: mh_capi.cpp (ckpt_device.hpp).
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/mcmcdate_mvn.h"
#include "ckpt_device.hpp"

extern "C" int mcd_set_last_error_(int code, const char* msg);   // mvn_capi.cpp

namespace {

int cfail(int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    return mcd_set_last_error_(code, buf);
}

#define CHIP_TRY(expr)                                                                             \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess) return cfail(MCD_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_));   \
    } while (0)

uint64_t bits(double x)
{
    uint64_t w;
    memcpy(&w, &x, 8);
    return w;
}

// the configuration's hashes: the checksum of the words (n_nodes, parent[]) and of (n_prop, the rows' eight columns)
uint64_t topology_hash(int n_nodes, const int32_t* parent)
{
    std::vector<uint64_t> w{(uint64_t)n_nodes};
    for (int v = 0; v < n_nodes; ++v) w.push_back((uint64_t)(uint32_t)parent[v]);
    return mcd::ckpt_checksum(w.data(), w.size());
}

uint64_t table_hash(int n_prop, const mcd::MhRow* rows, const int32_t* dims)
{
    std::vector<uint64_t> w{(uint64_t)n_prop};
    for (int i = 0; i < n_prop; ++i) {
        const mcd::MhRow& r = rows[i];
        for (int32_t x : {r.kind, r.node, r.n1, r.n2, r.jac_root, dims[i]}) w.push_back((uint64_t)(uint32_t)x);
        w.push_back(bits(r.p0));
        w.push_back(bits(r.p1));
    }
    return mcd::ckpt_checksum(w.data(), w.size());
}

// the blob of a handle as it stands: header words (the table's checksums 0), META, and the job that moves the device sections
struct Layout {
    int n = 0;
    uint64_t header_words = 0, total_words = 0;
    std::vector<uint64_t> header;             // header_words words, the last (the header's checksum) 0
    uint64_t meta[mcd::kCkptMetaWords] = {};
    mcd::CkptJob job{};                       // sections 1 .. n - 1 of the table (META is written by the host); job.s[k] is table row k + 1
};

void add(Layout& L, uint32_t id, void* arr, int kind, uint64_t n_words, int64_t row_len, int64_t ld)
{
    L.header.push_back(id);
    L.header.push_back(n_words);              // (offsets once all sections are known)
    if (id != MCD_CKPT_SEC_META) L.job.s[L.job.n++] = mcd::CkptSec{arr, n_words, 0, row_len, ld, kind, 0};
    L.n += 1;
}

Layout layout_of(const mcd::CkptView& v)
{
    using namespace mcd;
    Layout L;
    const MhDev& D = v.dev;
    const uint64_t B = (uint64_t)D.batch, n = (uint64_t)D.n_nodes, P = (uint64_t)D.n_prop, BP = B * P;
    add(L, MCD_CKPT_SEC_META, nullptr, CKPT_WORDS, kCkptMetaWords, 0, 0);
    add(L, MCD_CKPT_SEC_SC, D.sc, CKPT_WORDS, 5 * B, 0, 0);
    add(L, MCD_CKPT_SEC_HEIGHTS, D.H, CKPT_ROWS, B * n, (int64_t)n, D.ld);
    add(L, MCD_CKPT_SEC_RATES, D.R, CKPT_ROWS, B * n, (int64_t)n, D.ld);
    add(L, MCD_CKPT_SEC_POST, D.post, CKPT_WORDS, 3 * B, 0, 0);
    add(L, MCD_CKPT_SEC_PCOMP, D.pcomp, CKPT_WORDS, 3 * B, 0, 0);
    add(L, MCD_CKPT_SEC_BETA, D.beta, CKPT_WORDS, B, 0, 0);
    add(L, MCD_CKPT_SEC_TUNE, D.tune, CKPT_WORDS, BP, 0, 0);
    add(L, MCD_CKPT_SEC_ACCEPTED, D.acc, CKPT_INT32, (BP + 1) / 2, (int64_t)BP, 0);
    add(L, MCD_CKPT_SEC_TRIED, D.tried, CKPT_INT32, (BP + 1) / 2, (int64_t)BP, 0);
    add(L, MCD_CKPT_SEC_AGE_SUM, D.age_sum, CKPT_WORDS, B * n, 0, 0);
    add(L, MCD_CKPT_SEC_AGE_SQ, D.age_sq, CKPT_WORDS, B * n, 0, 0);
    uint32_t flags = (v.dense ? MCD_CKPT_FLAG_DENSE : 0) | (v.rec_active ? MCD_CKPT_FLAG_RECORDER : 0) | (D.lik_only ? MCD_CKPT_FLAG_POWER : 0);
    if (v.mc3.n_chains != 0) {
        flags |= MCD_CKPT_FLAG_MC3;
        add(L, MCD_CKPT_SEC_MC3_RANK, v.mc3.rank, CKPT_INT32, ((uint64_t)v.mc3.total + 1) / 2, v.mc3.total, 0);
        add(L, MCD_CKPT_SEC_MC3_TRIED, v.mc3.tried, CKPT_WORDS, (uint64_t)v.mc3.n_chains - 1, 0, 0);
        add(L, MCD_CKPT_SEC_MC3_ACCEPTED, v.mc3.accepted, CKPT_WORDS, (uint64_t)v.mc3.n_chains - 1, 0, 0);
    }
    if (v.ham) {
        flags |= MCD_CKPT_FLAG_HAMILTONIAN | (v.ham_inv_mass ? MCD_CKPT_FLAG_INV_MASS : 0);
        add(L, MCD_CKPT_SEC_HAM_SUMS, v.ham_sums, CKPT_WORDS, 4 * B, 0, 0);
        add(L, MCD_CKPT_SEC_HAM_EPS, v.ham_eps, CKPT_WORDS, B, 0, 0);
        if (v.ham_inv_mass) add(L, MCD_CKPT_SEC_HAM_INV_MASS, v.ham_inv_mass, CKPT_WORDS, (uint64_t)v.ham_dim, 0, 0);
    }
    // the header: fixed words, then the table with the sections back to back behind the header
    const std::vector<uint64_t> secs = L.header;          // (id, words) pairs
    L.header_words = ckpt_header_words(L.n);
    L.header.assign(L.header_words, 0);
    uint64_t at = L.header_words;
    for (int s = 0; s < L.n; ++s) {
        uint64_t* row = L.header.data() + kCkptFixedWords + 4 * s;
        row[0] = secs[2 * s];
        row[1] = 8 * at;
        row[2] = 8 * secs[2 * s + 1];
        if (s > 0) L.job.s[s - 1].blob_word = at;
        at += secs[2 * s + 1];
    }
    L.total_words = at;
    uint64_t* h = L.header.data();
    h[CKPT_W_MAGIC] = kCkptMagic;
    h[CKPT_W_VERSION_HBYTES] = (uint64_t)kCkptVersion | (8 * L.header_words) << 32;
    h[CKPT_W_TOTAL] = 8 * L.total_words;
    h[CKPT_W_NSEC_FLAGS] = (uint64_t)L.n | (uint64_t)flags << 32;
    h[CKPT_W_NODES_PROPS] = (uint64_t)(uint32_t)D.n_nodes | (uint64_t)(uint32_t)D.n_prop << 32;
    h[CKPT_W_BATCH] = B;
    h[CKPT_W_DIM_DENSE] = (uint64_t)(uint32_t)v.dim | (uint64_t)(v.dense ? 1 : 0) << 32;
    h[CKPT_W_SEED] = v.seed;
    h[CKPT_W_CHAIN0] = (uint64_t)D.chain0;
    h[CKPT_W_TOPOLOGY] = topology_hash(D.n_nodes, v.host_parent);
    h[CKPT_W_TABLE] = table_hash(D.n_prop, v.rows, v.dims);
    h[CKPT_W_FINGERPRINT] = ckpt_checksum(h + CKPT_W_NODES_PROPS, CKPT_W_FINGERPRINT - CKPT_W_NODES_PROPS);
    h[CKPT_W_STEP] = v.step;
    uint64_t* m = L.meta;
    m[CKPT_M_STEP] = v.step;
    m[CKPT_M_N_SAMPLES] = (uint64_t)v.n_samples;
    m[CKPT_M_LIK_ONLY] = (uint64_t)D.lik_only;
    if (v.rec_active) {
        m[CKPT_M_REC_PERIOD] = (uint64_t)v.rec_period;
        m[CKPT_M_REC_ITER] = (uint64_t)v.rec_iter;
        m[CKPT_M_REC_FETCHED] = (uint64_t)v.rec_fetched;
    }
    if (v.mc3.n_chains != 0) {
        m[CKPT_M_MC3_CHAINS] = (uint64_t)v.mc3.n_chains;
        m[CKPT_M_MC3_TOTAL] = (uint64_t)v.mc3.total;
        m[CKPT_M_MC3_SEED] = v.mc3_seed;
        m[CKPT_M_MC3_PHASE] = v.mc3_phase;
        for (int i = 0; i < v.mc3.n_chains && i < 16; ++i) m[CKPT_M_MC3_LADDER + i] = bits(v.mc3_ladder[i]);
    }
    if (v.ham) {
        m[CKPT_M_HAM] = 1;
        m[CKPT_M_HAM_DEPTH] = (uint64_t)v.ham_depth;
        m[CKPT_M_HAM_SEED] = v.ham_seed;
        m[CKPT_M_HAM_NEXT] = v.ham_next;
        m[CKPT_M_HAM_COUNTED] = (uint64_t)v.ham_counted;
        m[CKPT_M_HAM_INV_MASS] = v.ham_inv_mass ? 1 : 0;
        m[CKPT_M_HAM_DIM] = (uint64_t)v.ham_dim;
    }
    return L;
}

}  // namespace

extern "C" {

uint64_t mcd_ckpt_checksum(const void* words, int64_t n_words) { return (words && n_words > 0) ? mcd::ckpt_checksum(words, (uint64_t)n_words) : 0; }

int mcd_ckpt_inspect(const void* buf, int64_t len, mcd_ckpt_info_t* info)
{
    if (!buf || !info) return cfail(MCD_ERR_INVALID_ARG, "mcd_ckpt_inspect: NULL argument");
    char why[256];
    if (mcd::ckpt_parse(buf, len, info, true, why, sizeof why)) return cfail(MCD_ERR_INVALID_ARG, "mcd_ckpt_inspect: %s", why);
    return MCD_OK;
}

int mcd_mh_save_size(const mcd_mh_t* m, int64_t* bytes)
{
    if (!m || !bytes) return cfail(MCD_ERR_INVALID_ARG, "mcd_mh_save_size: NULL argument");
    mcd::CkptView v;
    if (int rc = mcd_mh_ckpt_view_(m, &v)) return rc;
    *bytes = (int64_t)(8 * layout_of(v).total_words);
    return MCD_OK;
}

int mcd_mh_save(mcd_mh_t* m, void* buf, int64_t cap, int64_t* written)
{
    const char* who = "mcd_mh_save";
    if (written) *written = 0;
    if (!m || !buf) return cfail(MCD_ERR_INVALID_ARG, "%s: NULL argument", who);
    mcd::CkptView v;
    if (int rc = mcd_mh_ckpt_view_(m, &v)) return rc;
    if (!v.have_state) return cfail(MCD_ERR_INVALID_ARG, "%s: the handle has no state yet (mcd_mh_set_state or mcd_mh_load first)", who);
    if (v.rec_active && v.rec_iter / v.rec_period != v.rec_fetched)
        return cfail(MCD_ERR_INVALID_ARG, "%s: %lld samples are waiting in the recorder's ring, which is not saved: take them with mcd_mh_record_fetch first", who,
                     (long long)(v.rec_iter / v.rec_period - v.rec_fetched));
    Layout L = layout_of(v);
    const int64_t total = (int64_t)(8 * L.total_words);
    if (cap < total) {
        if (written) *written = total;
        return cfail(MCD_ERR_INVALID_ARG, "%s: the buffer holds %lld bytes, the checkpoint needs %lld", who, (long long)cap, (long long)total);
    }
    unsigned blocks = 0;
    void* stage = nullptr;
    if (!mcd::ckpt_plan(&L.job, &blocks)) return cfail(MCD_ERR_UNSUPPORTED, "%s: the handle's arrays are too large for one launch", who);
    if (int rc = mcd_mh_ckpt_stage_(m, (size_t)total, &stage)) return rc;
    CHIP_TRY(hipSetDevice(v.device));
    // the header's place and META stay 0 on the device; the sections' checksums are added up in the table's checksum words there
    const uint64_t head = L.header_words + mcd::kCkptMetaWords;
    CHIP_TRY(hipMemsetAsync(stage, 0, 8 * head, v.stream));
    L.job.blob = (uint64_t*)stage;
    L.job.sums = (unsigned long long*)stage + mcd::kCkptFixedWords + 4 + 3;   // table row 1, checksum word
    L.job.sum_stride = 4;
    CHIP_TRY(mcd::launch_ckpt_pack(L.job, blocks, v.stream));
    CHIP_TRY(hipMemcpyAsync(buf, stage, (size_t)total, hipMemcpyDeviceToHost, v.stream));
    CHIP_TRY(hipStreamSynchronize(v.stream));
    // the host's part: header words around the device's checksums, META and its checksum, the header's checksum
    for (int s = 1; s < L.n; ++s) L.header[mcd::kCkptFixedWords + 4 * s + 3] = mcd::ckpt_word(buf, mcd::kCkptFixedWords + 4 * s + 3);
    L.header[mcd::kCkptFixedWords + 3] = mcd::ckpt_checksum(L.meta, mcd::kCkptMetaWords);
    L.header[L.header_words - 1] = mcd::ckpt_checksum(L.header.data(), L.header_words - 1);
    memcpy(buf, L.header.data(), 8 * L.header_words);
    memcpy((unsigned char*)buf + 8 * L.header_words, L.meta, 8 * mcd::kCkptMetaWords);
    if (written) *written = total;
    return MCD_OK;
}

int mcd_mh_load(mcd_mh_t* m, const void* buf, int64_t len, int flags)
{
    using namespace mcd;
    const char* who = "mcd_mh_load";
    if (!m || !buf) return cfail(MCD_ERR_INVALID_ARG, "%s: NULL argument", who);
    if (flags != MCD_CKPT_FULL && flags != MCD_CKPT_STATE_TUNING) return cfail(MCD_ERR_INVALID_ARG, "%s: flags must be MCD_CKPT_FULL or MCD_CKPT_STATE_TUNING", who);
    const bool full = flags == MCD_CKPT_FULL;
    mcd_ckpt_info_t I;
    char why[256];
    if (ckpt_parse(buf, len, &I, false, why, sizeof why)) return cfail(MCD_ERR_INVALID_ARG, "%s: %s", who, why);
    CkptView v;
    if (int rc = mcd_mh_ckpt_view_(m, &v)) return rc;
    const Layout L = layout_of(v);
    const uint64_t* h = L.header.data();
    const MhDev& D = v.dev;
    uint64_t meta[kCkptMetaWords];
    memcpy(meta, (const unsigned char*)buf + I.section_offset[0], sizeof meta);
    // ---- the configuration: the mismatch is named, nothing has been touched ----
    if (I.n_nodes != D.n_nodes) return cfail(MCD_ERR_INVALID_ARG, "%s: the checkpoint's tree has %d nodes, the handle's %d", who, I.n_nodes, D.n_nodes);
    if (I.topology != h[CKPT_W_TOPOLOGY]) return cfail(MCD_ERR_INVALID_ARG, "%s: the checkpoint was saved over another topology of %d nodes", who, I.n_nodes);
    if (I.batch != D.batch) return cfail(MCD_ERR_INVALID_ARG, "%s: the checkpoint holds a batch of %lld chains, the handle %lld", who, (long long)I.batch, (long long)D.batch);
    if (I.n_prop != D.n_prop) return cfail(MCD_ERR_INVALID_ARG, "%s: the checkpoint's proposal table has %d rows, the handle's %d", who, I.n_prop, D.n_prop);
    if (full) {
        if ((I.dense != 0) != v.dense)
            return cfail(MCD_ERR_INVALID_ARG, "%s: the checkpoint was saved over a %s likelihood, the handle has a %s one", who, I.dense ? "dense" : "sparse", v.dense ? "dense" : "sparse");
        if (I.dim != v.dim) return cfail(MCD_ERR_INVALID_ARG, "%s: the checkpoint's likelihood has the dimension %d, the handle's %d", who, I.dim, v.dim);
        if (I.table != h[CKPT_W_TABLE]) return cfail(MCD_ERR_INVALID_ARG, "%s: the checkpoint was saved with another proposal table (a row's kind, node, n1, n2, jac_root, dim, p0 or p1 differs)", who);
        if (I.seed != v.seed) return cfail(MCD_ERR_INVALID_ARG, "%s: the checkpoint was saved with the seed %llu, the handle has %llu", who, (unsigned long long)I.seed, (unsigned long long)v.seed);
        if (I.chain0 != D.chain0) return cfail(MCD_ERR_INVALID_ARG, "%s: the checkpoint's first chain is %lld, the handle's %lld (mcd_mh_set_chain_offset)", who, (long long)I.chain0, (long long)D.chain0);
        if (I.fingerprint != h[CKPT_W_FINGERPRINT]) return cfail(MCD_ERR_INVALID_ARG, "%s: the checkpoint's configuration fingerprint differs from the handle's", who);
        // the recorder: same period or none on the handle; nothing waiting on either side
        if (v.rec_active && meta[CKPT_M_REC_PERIOD] != 0) {
            if ((int64_t)meta[CKPT_M_REC_PERIOD] != v.rec_period)
                return cfail(MCD_ERR_INVALID_ARG, "%s: the checkpoint's recorder has the period %lld, the handle's %d", who, (long long)meta[CKPT_M_REC_PERIOD], v.rec_period);
            if (meta[CKPT_M_REC_ITER] / meta[CKPT_M_REC_PERIOD] != meta[CKPT_M_REC_FETCHED])
                return cfail(MCD_ERR_INVALID_ARG, "%s: the checkpoint's recorder counts name waiting samples, which no blob holds", who);
            if (v.rec_iter / v.rec_period != v.rec_fetched)
                return cfail(MCD_ERR_INVALID_ARG, "%s: samples are waiting in the handle's ring and would be lost: take them with mcd_mh_record_fetch first", who);
        }
        // MC3 and the attachment: both sides or neither, set up alike
        const int bc = (int)meta[CKPT_M_MC3_CHAINS];
        if ((bc != 0) != (v.mc3.n_chains != 0))
            return cfail(MCD_ERR_INVALID_ARG, bc ? "%s: the checkpoint holds Metropolis-coupled MCMC; call mcd_mh_mc3_init on the handle first" : "%s: Metropolis-coupled MCMC is initialised on the handle, the checkpoint has none", who);
        if (bc != 0) {
            if (bc != v.mc3.n_chains || (int64_t)meta[CKPT_M_MC3_TOTAL] != v.mc3.total || meta[CKPT_M_MC3_SEED] != v.mc3_seed)
                return cfail(MCD_ERR_INVALID_ARG, "%s: the checkpoint's MC3 (n_chains %d, %lld chains in all, its seed) is not the handle's (n_chains %d, %lld)", who, bc,
                             (long long)meta[CKPT_M_MC3_TOTAL], v.mc3.n_chains, (long long)v.mc3.total);
            for (int i = 0; i < bc && i < 16; ++i)
                if (meta[CKPT_M_MC3_LADDER + i] != bits(v.mc3_ladder[i]))
                    return cfail(MCD_ERR_INVALID_ARG, "%s: the checkpoint's MC3 ladder differs from the handle's at rung %d", who, i);
        }
        const bool bh = meta[CKPT_M_HAM] != 0;
        if (bh != v.ham)
            return cfail(MCD_ERR_INVALID_ARG, bh ? "%s: the checkpoint holds an attached Hamiltonian proposal; call mcd_mh_attach_hamiltonian on the handle first" : "%s: a Hamiltonian proposal is attached to the handle, the checkpoint has none", who);
        if (bh && ((int)meta[CKPT_M_HAM_DEPTH] != v.ham_depth || meta[CKPT_M_HAM_SEED] != v.ham_seed || (meta[CKPT_M_HAM_INV_MASS] != 0) != (v.ham_inv_mass != nullptr) ||
                   (int)meta[CKPT_M_HAM_DIM] != v.ham_dim))
            return cfail(MCD_ERR_INVALID_ARG, "%s: the checkpoint's attachment (max_depth %d, its seed, inv_mass %s) is not the handle's (max_depth %d, inv_mass %s)", who,
                         (int)meta[CKPT_M_HAM_DEPTH], meta[CKPT_M_HAM_INV_MASS] ? "given" : "NULL", v.ham_depth, v.ham_inv_mass ? "given" : "NULL");
        if (v.ham && (meta[CKPT_M_LIK_ONLY] != 0 || bc != 0))
            return cfail(MCD_ERR_UNSUPPORTED, "%s: a Hamiltonian proposal is attached to the handle: no MC3, no power posterior", who);
        // with the configuration equal, the table must be the handle's own, row for row
        if (I.n_sections != L.n) return cfail(MCD_ERR_INVALID_ARG, "%s: the checkpoint has %d sections, the handle's layout %d", who, I.n_sections, L.n);
        for (int s = 0; s < L.n; ++s)
            if ((uint64_t)I.section_id[s] != h[kCkptFixedWords + 4 * s] || (uint64_t)I.section_offset[s] != h[kCkptFixedWords + 4 * s + 1] ||
                (uint64_t)I.section_bytes[s] != h[kCkptFixedWords + 4 * s + 2])
                return cfail(MCD_ERR_INVALID_ARG, "%s: section %d of the checkpoint (id %d, %lld bytes) is not what the handle's layout has there", who, s, I.section_id[s],
                             (long long)I.section_bytes[s]);
    }
    // ---- the jobs: every section of the BLOB's table is summed; the handle's arrays take the sections they have in common ----
    CkptJob verify{}, unpack{};
    verify.n = I.n_sections;
    for (int s = 0; s < I.n_sections; ++s) verify.s[s] = CkptSec{nullptr, (uint64_t)I.section_bytes[s] / 8, (uint64_t)I.section_offset[s] / 8, 0, 0, CKPT_WORDS, 0};
    for (int k = 0; k < L.job.n; ++k) {
        const int id = (int)h[kCkptFixedWords + 4 * (k + 1)];
        const bool wanted = full || id == MCD_CKPT_SEC_SC || id == MCD_CKPT_SEC_HEIGHTS || id == MCD_CKPT_SEC_RATES || id == MCD_CKPT_SEC_POST ||
                            id == MCD_CKPT_SEC_PCOMP || id == MCD_CKPT_SEC_TUNE;
        if (!wanted) continue;
        int at = -1;
        for (int s = 0; s < I.n_sections; ++s)
            if (I.section_id[s] == id) at = s;
        if (at < 0 || (uint64_t)I.section_bytes[at] != 8 * L.job.s[k].n_words)
            return cfail(MCD_ERR_INVALID_ARG, "%s: the checkpoint's section %d is missing or has another size than the handle's array", who, id);
        CkptSec S = L.job.s[k];
        S.blob_word = (uint64_t)I.section_offset[at] / 8;
        unpack.s[unpack.n++] = S;
    }
    unsigned vblocks = 0, ublocks = 0;
    if (!ckpt_plan(&verify, &vblocks) || !ckpt_plan(&unpack, &ublocks)) return cfail(MCD_ERR_UNSUPPORTED, "%s: the checkpoint is too large for one launch", who);
    // ---- device: copy, verify, compare, unpack ----
    void* stage = nullptr;
    const size_t sums_at = ((size_t)len + 7) / 8 * 8;
    if (int rc = mcd_mh_ckpt_stage_(m, sums_at + 8 * kCkptMaxSections, &stage)) return rc;
    CHIP_TRY(hipSetDevice(v.device));
    unsigned long long* d_sums = (unsigned long long*)((unsigned char*)stage + sums_at);
    unsigned long long sums[kCkptMaxSections];
    CHIP_TRY(hipMemcpyAsync(stage, buf, (size_t)len, hipMemcpyHostToDevice, v.stream));
    CHIP_TRY(hipMemsetAsync(d_sums, 0, sizeof sums, v.stream));
    verify.blob = unpack.blob = (uint64_t*)stage;
    verify.sums = d_sums;
    verify.sum_stride = 1;
    CHIP_TRY(launch_ckpt_verify(verify, vblocks, v.stream));
    CHIP_TRY(hipMemcpyAsync(sums, d_sums, sizeof sums, hipMemcpyDeviceToHost, v.stream));
    CHIP_TRY(hipStreamSynchronize(v.stream));
    for (int s = 0; s < I.n_sections; ++s)
        if (sums[s] != I.section_checksum[s])
            return cfail(MCD_ERR_INVALID_ARG, "%s: section %d (id %d): its checksum does not match its bytes", who, s, I.section_id[s]);
    CHIP_TRY(launch_ckpt_unpack(unpack, ublocks, v.stream));
    if (!full) {
        const size_t BP = (size_t)D.batch * (size_t)D.n_prop;
        CHIP_TRY(hipMemsetAsync(D.acc, 0, sizeof(int32_t) * BP, v.stream));
        CHIP_TRY(hipMemsetAsync(D.tried, 0, sizeof(int32_t) * BP, v.stream));
    }
    CHIP_TRY(hipStreamSynchronize(v.stream));
    CkptCommit c{};
    c.full = full;
    c.step = meta[CKPT_M_STEP];
    c.n_samples = (int64_t)meta[CKPT_M_N_SAMPLES];
    c.lik_only = (int32_t)meta[CKPT_M_LIK_ONLY];
    c.rec = v.rec_active && meta[CKPT_M_REC_PERIOD] != 0;
    c.rec_iter = (int64_t)meta[CKPT_M_REC_ITER];
    c.rec_fetched = (int64_t)meta[CKPT_M_REC_FETCHED];
    c.mc3_phase = meta[CKPT_M_MC3_PHASE];
    c.ham_next = meta[CKPT_M_HAM_NEXT];
    c.ham_counted = (int64_t)meta[CKPT_M_HAM_COUNTED];
    return mcd_mh_ckpt_commit_(m, c);
}

}  // extern "C"
