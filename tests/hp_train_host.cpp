// Test shim (CPU tests only): the engine's homopolymer walk (nanosim_amd/csrc/ns_hp_hist.h — the code k_hp_count and k_hp_records run
// per thread) compiled for the HOST behind the signature of ns_hp_histograms, so that the walk and the host module around the call are
// checked against the reference's fixture without a GPU.  Built by tests/test_hp_train.py with g++ into tests/_tmp/.
#include <stdint.h>
#include <string.h>
#include "../include/nanosim_amd.h"
#include "../nanosim_amd/csrc/ns_hp_hist.h"

struct HostHpAcc {
    ns_hp_hist *out; uint32_t aln; bool write;
    void hp(uint32_t cls, uint8_t base, uint32_t ref_len, uint32_t read_len, uint32_t start, uint32_t) {
        if (write) {
            const uint32_t code = base == 'A' ? 0u : base == 'C' ? 1u : base == 'G' ? 2u : 3u;
            out->records[out->n_hp] = ns_hp_record{aln, start, ref_len, read_len << 2 | code};
        }
        out->n_hp += 1;
        if (write) return;
        if (ref_len > out->max_ref) out->max_ref = ref_len;
        if (read_len > out->max_read) out->max_read = read_len;
        if (ref_len < out->cap_ref && read_len < out->cap_read) out->table[((uint64_t)cls * out->cap_ref + ref_len) * out->cap_read + read_len] += 1;
        else out->n_overflow += 1;
    }
    void columns(uint32_t ins, uint32_t del, uint32_t mis, uint32_t match) {
        if (write) return;
        out->columns[0] += ins; out->columns[1] += del; out->columns[2] += mis; out->columns[3] += match;
    }
};

extern "C" int hp_host_histograms(void *, const uint8_t *ref, const uint8_t *qry, uint64_t nbytes, const uint64_t *off, uint32_t n_aln,
                                  uint32_t min_hp_len, ns_hp_hist *out) {
    if (!out || !out->table || !min_hp_len || !out->cap_ref || !out->cap_read) return -1;
    for (uint32_t a = 0; a < n_aln; ++a) if (off[a] > off[a + 1] || off[a + 1] > nbytes) return -1;
    out->n_hp = out->max_ref = out->max_read = out->n_overflow = 0; out->ms_kernel = 0;
    memset(out->columns, 0, sizeof out->columns);
    memset(out->table, 0, (size_t)2 * out->cap_ref * out->cap_read * 8);
    for (uint32_t a = 0; a < n_aln; ++a) {
        HostHpAcc acc{out, a, false};
        const uint8_t *r = ref + off[a], *q = qry + off[a];
        hp_hist_alignment(r, q, off[a + 1] - off[a], min_hp_len, acc);
    }
    if (!out->records || out->n_hp > out->cap_records) return 0;
    out->n_hp = 0;                                                              // the second pass counts them again while it writes
    for (uint32_t a = 0; a < n_aln; ++a) {
        HostHpAcc acc{out, a, true};
        const uint8_t *r = ref + off[a], *q = qry + off[a];
        hp_hist_alignment(r, q, off[a + 1] - off[a], min_hp_len, acc);
    }
    return 0;
}

// read_len of a read segment alone: the restated `(BB+){s<=1}` scan
extern "C" uint32_t hp_host_fuzzy_len(const uint8_t *seg, uint64_t n, uint8_t base) { return hp_fuzzy_len(seg, n, base); }

#ifdef HP_MAIN
// The walk as a stand-alone program for -fsanitize=address,undefined (tests/test_hp_train.py): the pairs of a file, `reference-line
// query-line` per row, in exact-size buffers; prints n_hp, the four column sums, max_ref and max_read for the k of argv[2].
#include <stdio.h>
#include <stdlib.h>
#include <string>
#include <vector>
int main(int argc, char **argv) {
    if (argc < 3) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    std::vector<uint8_t> ref, qry; std::vector<uint64_t> off{0};
    std::vector<char> a(1 << 20), b(1 << 20);
    while (fscanf(f, "%1048575s %1048575s", a.data(), b.data()) == 2) {
        if (strlen(a.data()) != strlen(b.data())) return 2;
        ref.insert(ref.end(), a.data(), a.data() + strlen(a.data()));
        qry.insert(qry.end(), b.data(), b.data() + strlen(b.data()));
        off.push_back(ref.size());
    }
    fclose(f);
    const uint32_t cap = 64;
    std::vector<uint64_t> table((size_t)2 * cap * cap);
    ns_hp_hist h; memset(&h, 0, sizeof h);
    h.table = table.data(); h.cap_ref = h.cap_read = cap;
    if (hp_host_histograms(nullptr, ref.data(), qry.data(), ref.size(), off.data(), (uint32_t)off.size() - 1u, (uint32_t)atoi(argv[2]), &h)) return 3;
    printf("%llu %llu %llu %llu %llu %u %u\n", (unsigned long long)h.n_hp, (unsigned long long)h.columns[0], (unsigned long long)h.columns[1],
           (unsigned long long)h.columns[2], (unsigned long long)h.columns[3], h.max_ref, h.max_read);
    return 0;
}
#endif
