// ns_calmd.h — training side, tags from the reference genome ("cs and MD from the reference"): the MD:Z text (samtools calmd's
// algorithm) and the short-form cs:Z text (minimap2 --cs) of an alignment from its CIGAR, its POS, its SEQ and the engine's normalised
// copy of the reference.  The reference assumes its own `minimap2 --cs` run (src/besthit_to_histogram.py:320-324); the files people have
// carry neither tag, often with = / X ops.
//
// The rules of the text.
//   Columns     the columns of an alignment are those of its M, = and X ops; adjacent ops of the three kinds are one run of columns.  What
//               the letter of the op claims is ignored: the bases decide.
//   Match       a column is a match when the SEQ letter and the reference letter are equal after upper-casing and neither is N.  The
//               reference is the engine's copy: upper case, what is no IUPAC code is N (bit 7, which marks the codes there, is dropped).
//   MD          u counts the match columns since the last item.  A mismatch column writes u, the reference letter in upper case, u = 0.
//               Every D op writes u, `^`, its reference letters in upper case, u = 0.  The end writes u.  I, S and H write nothing and do
//               not reset u: 10M2I10M on matching bases is `20`.  Two mismatches in a row: `A0C`; a mismatch behind a deletion: `^AC0T`;
//               two D ops in a row: `^AC0^G`.
//   cs          `:n` per maximal run of match columns (an I or D op or a mismatch ends it; n is never 0), `*<ref><read>` per mismatch
//               column, `+<read letters>` per I op, `-<ref letters>` per D op, all letters in lower case; clips write nothing.
//               (minimap2's own treatment of ambiguity codes in cs is not verified: DESIGN §9.)
//   Bad records get empty texts and a reason, the first of: the reference index is outside the set reference (CALMD_BAD_CHROM); POS is 0
//               (_POS); then along the CIGAR, byte by byte: it does not parse — a byte that is neither a digit nor a letter nor `=`, an op
//               without a count, a count of 0, of more than CALMD_MAX_DIGITS digits or of 2^28 or more, sums of 2^31 or more, digits at the
//               end, no byte at all (_CIGAR); an op outside MIDSH=X (_OP; N and P are not handled, as in ns_sam_pairs.h); an S that is not
//               outermost inside the H ops, or an H that is not outermost (_CLIP); then no M / = / X column at all (_NO_COLUMN); a SEQ
//               whose length is not the sum of its S/M/=/X/I ops (_SEQ_LEN); an alignment that runs past the end of its chromosome (_END);
//               a SEQ byte that is not a letter (_SEQ_BYTE).  Nothing of the reference is read for a bad record.
//
// What is built.  ONE WAVEFRONT PER RECORD (W::LANES lanes; the host build runs the same code with one lane), two walks:
//   ops      (calmd_ops)  the CIGAR text W::LANES BYTES at a time.  A ballot gives the mask of the op letters; the count of an op is the
//            digits between its letter and the letter below it in the mask (or the last letter of the round before), read by the op's
//            lane.  The order of the clips is checked on the masks of H, S and the other ops with four flags carried between rounds.
//            Three prefix sums over the wavefront turn the ops into what stands in front of each — columns, SEQ bytes, reference letters —
//            and every op goes to the record's table (CalmdOp; room for one op per two CIGAR bytes).  No lane walks the ops.
//   text     (calmd_text) the COLUMNS, W::LANES per step, plus one virtual column behind the last for what ends the text.  A lane finds
//            the op of its column by bisection in the table (from the op of the step's first column on), so an indel every 10-20 columns
//            costs no step: SEQ and reference are loaded one byte per lane, neighbours next to each other wherever an op goes on.  The
//            mismatch mask X is a ballot; so are Bd and Bi, the columns in front of which one or more D, or I or D, ops stand.  The match
//            run that ends at a column is its lane number minus the highest bit of (X << 1 | B) at or below it, or the lane number plus
//            the run carried in from the steps before when there is none: no loop, and the digit counts follow.  The bytes of a column
//            — the run that ends in front of its indel ops, those ops, the run and the letters of its mismatch — go through a prefix
//            sum; measure (WRITE = false) stops there, write stores them.  The letters of an indel group are stored by the lane of the
//            column behind it, one loop per group: an insertion of kilobases is one lane's work (a known weakness; ONT indels are
//            1-3 letters).
// The SEQ letters are checked 8 bytes per lane.  Every reference load lies inside the chromosome (checked against the ops' sum before
// the first), every SEQ load inside the record's SEQ (its length is the ops' sum), every store inside the measured text (checked per
// lane; calmd_text<true> returns false when the two walks disagree).
// W, the wavefront: lane, ballot (64-bit mask of a predicate), scan (exclusive prefix sum + total, 64-bit), bcast (a lane's value),
// fence (the table written by the lanes is read by other lanes of the same wavefront).
#pragma once
#include <stdint.h>
#include "ns_bam.h"

#define CALMD_MAX_DIGITS 9u          // of an op's count
#define CALMD_MAX_OPLEN (1u << 28)   // a count is below this (BAM's 28 bits)
#define CALMD_MAX_TOTAL (1ull << 31) // columns, SEQ bytes and reference letters of a record are below this
#define CALMD_SEQ_BYTES 8u           // SEQ bytes per lane and round of the letter check

enum { CALMD_OK = 0, CALMD_BAD_CIGAR = 1, CALMD_BAD_OP = 2, CALMD_BAD_CLIP = 3, CALMD_BAD_SEQ_LEN = 4, CALMD_BAD_SEQ_BYTE = 5, CALMD_BAD_CHROM = 6,
       CALMD_BAD_POS = 7, CALMD_BAD_END = 8, CALMD_BAD_NO_COLUMN = 9 };
enum { CALMD_M = 0, CALMD_I = 1, CALMD_D = 2, CALMD_S = 3, CALMD_H = 4, CALMD_NONE = 7 };     // (= and X are M)

struct CalmdOp { uint32_t kind_len, col, seq, ref; };                // kind << 28 | count; the columns, SEQ bytes, reference letters in front
struct CalmdRec { uint32_t first_op, end_op, n_cols, reason; };      // the ops of the columns and of the indels between them: [first_op, end_op)
struct CalmdRef { const uint8_t *bases; const uint64_t *chrom_off; uint32_t nchrom; };
// where the table of record r begins: ops <= CIGAR bytes / 2 (+ r: the halves round down)
NS_CSH uint64_t calmd_op_base(const uint64_t *cigar_off, uint64_t r) { return (cigar_off[r] >> 1) + r; }

NS_CSH uint32_t calmd_hi(uint64_t m) { return 63u - (uint32_t)__builtin_clzll(m); }          // the highest set bit (m != 0)
NS_CSH uint32_t calmd_kind(uint32_t kind_len) { return kind_len >> 28; }
NS_CSH uint32_t calmd_len(uint32_t kind_len) { return kind_len & (CALMD_MAX_OPLEN - 1u); }
NS_CSH bool calmd_is_letter(uint32_t c) { return ((c | 0x20u) - 'a') < 26u; }
NS_CSH uint32_t calmd_kind_of(uint8_t c) {
    return (c == 'M' || c == '=' || c == 'X') ? (uint32_t)CALMD_M : c == 'I' ? (uint32_t)CALMD_I : c == 'D' ? (uint32_t)CALMD_D : c == 'S' ? (uint32_t)CALMD_S :
           c == 'H' ? (uint32_t)CALMD_H : (uint32_t)CALMD_NONE;
}

// ---- ops: the CIGAR text cg[0 .. cn) into the table T; CALMD_OK with R.first_op / end_op / n_cols and the sums, or why it is bad ----
template <class W> NS_CSH uint32_t calmd_ops(W &w, const uint8_t *cg, uint64_t cn, CalmdOp *T, CalmdRec &R, uint64_t &seq_total, uint64_t &ref_total) {
    const uint64_t lt = (1ull << w.lane) - 1ull;                     // the lanes below mine
    int64_t last_letter = -1;                                        // the last op letter of the rounds before
    uint32_t n_ops = 0, first_op = ~0u, end_op = 0;
    bool seen_a = false, seen_lead = false, seen_trail = false, closed = false;     // an M/I/D op; an S in front of them; one behind; an H that is not op 0
    uint64_t col = 0, seq = 0, ref = 0;
    for (uint64_t cb = 0; cb < cn; cb += W::LANES) {
        const uint64_t p = cb + w.lane;
        const bool in = p < cn;
        const uint8_t ch = in ? cg[p] : (uint8_t)'0';
        const bool let = in && !(ch >= '0' && ch <= '9');
        const uint64_t mL = w.ballot(let);
        if (!mL) continue;                                           // digits only
        const uint32_t kind = let ? calmd_kind_of(ch) : (uint32_t)CALMD_NONE;
        uint32_t v = 0, reason = CALMD_OK;
        if (let) {
            const uint64_t below = mL & lt;
            const int64_t prev = below ? (int64_t)(cb + calmd_hi(below)) : last_letter;
            const uint64_t nd = p - (uint64_t)(prev + 1);
            if (kind == CALMD_NONE && !calmd_is_letter(ch)) reason = CALMD_BAD_CIGAR;
            else if (nd == 0 || nd > CALMD_MAX_DIGITS) reason = CALMD_BAD_CIGAR;
            else {
                for (uint64_t k = 0; k < nd; ++k) v = v * 10u + (uint32_t)(cg[(uint64_t)(prev + 1) + k] - '0');
                if (v == 0 || v >= CALMD_MAX_OPLEN) reason = CALMD_BAD_CIGAR;
                else if (kind == CALMD_NONE) reason = CALMD_BAD_OP;
            }
        }
        const bool is_a = kind == CALMD_M || kind == CALMD_I || kind == CALMD_D;
        const uint64_t mA = w.ballot(is_a), mS = w.ballot(kind == CALMD_S), mH = w.ballot(kind == CALMD_H);
        const uint64_t first_bit = n_ops ? 0ull : (mL & (0ull - mL)), low_a = mA & (0ull - mA);
        const uint64_t s_lead = seen_a ? 0ull : (mS & (low_a ? low_a - 1ull : ~0ull)), s_trail = seen_a ? mS : (low_a ? mS & ~(low_a - 1ull) : 0ull);
        const uint64_t h_closing = mH & ~first_bit;
        if (let && !reason) {                                        // the order of the clips, from what stands below me
            const bool a_before = seen_a || (mA & lt), trail_before = seen_trail || (s_trail & lt), lead_before = seen_lead || (s_lead & lt);
            if (closed || (h_closing & lt)) reason = CALMD_BAD_CLIP;
            else if (is_a && trail_before) reason = CALMD_BAD_CLIP;
            else if (kind == CALMD_S && (a_before ? trail_before : lead_before)) reason = CALMD_BAD_CLIP;
        }
        const uint64_t lc = kind == CALMD_M ? v : 0u, lq = (kind == CALMD_M || kind == CALMD_I || kind == CALMD_S) ? v : 0u,
                       lr = (kind == CALMD_M || kind == CALMD_D) ? v : 0u;
        uint64_t tc, tq, tr;
        const uint64_t ec = w.scan(lc, tc), eq = w.scan(lq, tq), er = w.scan(lr, tr);
        if (let && !reason && (col + ec + lc >= CALMD_MAX_TOTAL || seq + eq + lq >= CALMD_MAX_TOTAL || ref + er + lr >= CALMD_MAX_TOTAL)) reason = CALMD_BAD_CIGAR;
        const uint64_t e1 = w.ballot(reason == CALMD_BAD_CIGAR), e2 = w.ballot(reason == CALMD_BAD_OP), e3 = w.ballot(reason == CALMD_BAD_CLIP);
        if (const uint64_t any = e1 | e2 | e3) {                     // the lowest byte decides
            const uint64_t low = any & (0ull - any);
            return (e1 & low) ? CALMD_BAD_CIGAR : (e2 & low) ? CALMD_BAD_OP : CALMD_BAD_CLIP;
        }
        if (let) T[n_ops + (uint32_t)__builtin_popcountll(mL & lt)] = CalmdOp{kind << 28 | v, (uint32_t)(col + ec), (uint32_t)(seq + eq), (uint32_t)(ref + er)};
        if (mA) {
            if (first_op == ~0u) first_op = n_ops + (uint32_t)__builtin_popcountll(mL & (low_a - 1ull));
            const uint64_t hi_a = 1ull << calmd_hi(mA);
            end_op = n_ops + (uint32_t)__builtin_popcountll(mL & ((hi_a << 1) - 1ull));
        }
        seen_trail = seen_trail || s_trail; seen_lead = seen_lead || s_lead; closed = closed || h_closing; seen_a = seen_a || mA;
        last_letter = (int64_t)(cb + calmd_hi(mL));
        n_ops += (uint32_t)__builtin_popcountll(mL);
        col += tc; seq += tq; ref += tr;
    }
    if (!cn || last_letter != (int64_t)cn - 1) return CALMD_BAD_CIGAR;
    if (!col) return CALMD_BAD_NO_COLUMN;
    R.first_op = first_op; R.end_op = end_op; R.n_cols = (uint32_t)col; R.reason = CALMD_OK;
    seq_total = seq; ref_total = ref;
    return CALMD_OK;
}

// every byte of seq[0 .. sn) is a letter
template <class W> NS_CSH bool calmd_seq_letters(W &w, const uint8_t *seq, uint64_t sn) {
    bool bad = false;
    for (uint64_t i = (uint64_t)CALMD_SEQ_BYTES * w.lane; i < sn; i += (uint64_t)CALMD_SEQ_BYTES * W::LANES) {
        if (i + CALMD_SEQ_BYTES <= sn) {
            const uint64_t v = bam_u64(seq + i);
            for (uint32_t k = 0; k < CALMD_SEQ_BYTES; ++k) bad = bad || !calmd_is_letter((uint32_t)(v >> (8u * k)) & 0xffu);
        } else {
            for (uint64_t k = i; k < sn; ++k) bad = bad || !calmd_is_letter(seq[k]);
        }
    }
    return w.ballot(bad) == 0ull;
}

// the match run that ends in front of lane `lane`: starts = the columns at or below it at which a run begins
NS_CSH uint64_t calmd_run(uint64_t starts, uint32_t lane, uint64_t carry) { return starts ? (uint64_t)(lane - calmd_hi(starts)) : (uint64_t)lane + carry; }
NS_CSH uint64_t calmd_carry(uint64_t X, uint64_t starts, uint32_t lanes, uint64_t carry) {          // ... and what a whole step hands to the next
    if ((X >> (lanes - 1u)) & 1ull) return 0u;
    if (lanes < 64u) starts &= (1ull << lanes) - 1ull;
    return starts ? (uint64_t)(lanes - calmd_hi(starts)) : carry + lanes;
}

// ---- text: the two texts of a record whose ops are in T.  seq: its SEQ; ref: the reference at its POS.  WRITE false: the lengths to
// md_out / cs_out.  WRITE true: the texts to md[0 .. md_len) and cs[0 .. cs_len); false when they are not what was measured ----
template <bool WRITE, class W> NS_CSH bool calmd_text(W &w, const CalmdOp *T, const CalmdRec &R, const uint8_t *seq, const uint8_t *ref, uint8_t *md,
                                                      uint64_t md_len, uint8_t *cs, uint64_t cs_len, uint64_t &md_out, uint64_t &cs_out) {
    const uint64_t lt = (1ull << w.lane) - 1ull, le = (2ull << w.lane) - 1ull;          // the lanes below mine; and mine
    const uint64_t n_cols = R.n_cols;
    uint64_t md_pos = 0, cs_pos = 0, md_carry = 0, cs_carry = 0;
    uint32_t op_lo = R.first_op;                                     // the op of the step's first column
    bool ok = true;
    for (uint64_t base = 0; base <= n_cols; base += W::LANES) {
        const uint64_t c = base + w.lane;
        const bool real = c < n_cols, endc = c == n_cols;
        uint32_t j = R.end_op, k = 0;
        CalmdOp e = CalmdOp{0u, 0u, 0u, 0u};
        if (real) {                                                  // the last op whose columns begin at or in front of c: an M op
            uint32_t lo = op_lo, hi = R.end_op - 1u;
            while (lo < hi) { const uint32_t mid = lo + (hi - lo + 1u) / 2u; if (T[mid].col <= c) lo = mid; else hi = mid - 1u; }
            j = lo; e = T[j]; k = (uint32_t)c - e.col;
        }
        // the indel ops in front of the column: [g0, j)
        uint32_t g0 = j, n_del = 0;
        uint64_t gap_md = 0, gap_cs = 0;
        if (endc || (real && k == 0u)) {
            while (g0 > R.first_op) {
                const uint32_t kl = T[g0 - 1u].kind_len, kind = calmd_kind(kl);
                if (kind != CALMD_I && kind != CALMD_D) break;
                --g0;
                gap_cs += 1u + calmd_len(kl);
                if (kind == CALMD_D) { gap_md += 1u + calmd_len(kl); ++n_del; }
            }
            if (n_del) gap_md += n_del - 1u;                         // the `0` between two D ops
        }
        const bool bnd = g0 < j;
        uint8_t s = 0, r = 0;
        bool mis = false;
        if (real) { s = seq[(uint64_t)e.seq + k]; r = (uint8_t)(ref[(uint64_t)e.ref + k] & 0x7fu); mis = !((uint8_t)(s & 0xdfu) == r && r != 'N'); }
        const uint64_t X = w.ballot(mis), Bd = w.ballot(bnd && n_del), Bi = w.ballot(bnd), XS = X << 1;
        // MD: the run in front of the indel ops, the run in front of the column
        const uint64_t r1 = calmd_run((XS & le) | (Bd & lt), w.lane, md_carry), r2 = calmd_run((XS | Bd) & le, w.lane, md_carry);
        const uint32_t md_f1 = (bnd && n_del) ? bam_dec_len((uint32_t)r1) : 0u, md_d2 = (mis || endc) ? bam_dec_len((uint32_t)r2) : 0u;
        const uint64_t md_bytes = (uint64_t)md_f1 + gap_md + md_d2 + (mis ? 1u : 0u);
        // cs likewise; a run of 0 is not written
        const uint64_t n1 = calmd_run((XS & le) | (Bi & lt), w.lane, cs_carry), n2 = calmd_run((XS | Bi) & le, w.lane, cs_carry);
        const uint32_t cs_f1 = (bnd && n1) ? 1u + bam_dec_len((uint32_t)n1) : 0u, cs_d2 = ((mis || endc) && n2) ? 1u + bam_dec_len((uint32_t)n2) : 0u;
        const uint64_t cs_bytes = (uint64_t)cs_f1 + gap_cs + cs_d2 + (mis ? 3u : 0u);
        uint64_t md_total, cs_total;
        const uint64_t md_at = md_pos + w.scan(md_bytes, md_total), cs_at = cs_pos + w.scan(cs_bytes, cs_total);
        if (WRITE) {
            if (md_at + md_bytes > md_len || cs_at + cs_bytes > cs_len) ok = false;
            else if (md_bytes | cs_bytes) {
                uint8_t *q = md + md_at, *z = cs + cs_at;
                if (md_f1) { bam_put_dec(q, (uint32_t)r1, md_f1); q += md_f1; }
                if (cs_f1) { *z++ = ':'; bam_put_dec(z, (uint32_t)n1, cs_f1 - 1u); z += cs_f1 - 1u; }
                bool first_del = true;
                for (uint32_t g = g0; g < j; ++g) {
                    const CalmdOp o = T[g];
                    const uint32_t len = calmd_len(o.kind_len);
                    if (calmd_kind(o.kind_len) == CALMD_D) {
                        if (!first_del) *q++ = '0';
                        first_del = false;
                        *q++ = '^'; *z++ = '-';
                        for (uint32_t t = 0; t < len; ++t) { const uint8_t b = (uint8_t)(ref[(uint64_t)o.ref + t] & 0x7fu); *q++ = b; *z++ = (uint8_t)(b | 0x20u); }
                    } else {
                        *z++ = '+';
                        for (uint32_t t = 0; t < len; ++t) *z++ = (uint8_t)(seq[(uint64_t)o.seq + t] | 0x20u);
                    }
                }
                if (md_d2) { bam_put_dec(q, (uint32_t)r2, md_d2); q += md_d2; }
                if (cs_d2) { *z++ = ':'; bam_put_dec(z, (uint32_t)n2, cs_d2 - 1u); z += cs_d2 - 1u; }
                if (mis) { *q = r; z[0] = '*'; z[1] = (uint8_t)(r | 0x20u); z[2] = (uint8_t)(s | 0x20u); }
            }
        }
        md_pos += md_total; cs_pos += cs_total;
        if (base + W::LANES <= n_cols) {                             // a whole step of columns: what it hands on
            md_carry = calmd_carry(X, XS | Bd, W::LANES, md_carry);
            cs_carry = calmd_carry(X, XS | Bi, W::LANES, cs_carry);
            op_lo = w.bcast(j, W::LANES - 1u);
        }
    }
    md_out = md_pos; cs_out = cs_pos;
    if (WRITE) return w.ballot(!ok) == 0ull && md_pos == md_len && cs_pos == cs_len;
    return true;
}

// ---- measure: the record is checked, its ops go to T, its texts are measured.  CALMD_OK, or why it is bad (lengths 0) ----
template <class W> NS_CSH uint32_t calmd_measure(W &w, const uint8_t *cg, uint64_t cn, const uint8_t *seq, uint64_t sn, uint32_t chrom, uint32_t pos,
                                                 const CalmdRef &G, CalmdOp *T, CalmdRec &R, uint64_t &md_len, uint64_t &cs_len) {
    R = CalmdRec{0u, 0u, 0u, CALMD_OK};
    md_len = cs_len = 0;
    if (chrom >= G.nchrom) return R.reason = CALMD_BAD_CHROM;
    if (!pos) return R.reason = CALMD_BAD_POS;
    uint64_t seq_total = 0, ref_total = 0;
    if (const uint32_t reason = calmd_ops(w, cg, cn, T, R, seq_total, ref_total)) return R.reason = reason;
    if (seq_total != sn) return R.reason = CALMD_BAD_SEQ_LEN;
    const uint64_t c0 = G.chrom_off[chrom], c_len = G.chrom_off[chrom + 1u] - c0;
    if ((uint64_t)pos - 1u + ref_total > c_len) return R.reason = CALMD_BAD_END;
    if (!calmd_seq_letters(w, seq, sn)) return R.reason = CALMD_BAD_SEQ_BYTE;
    w.fence();
    calmd_text<false>(w, T, R, seq, G.bases + c0 + (pos - 1u), nullptr, 0, nullptr, 0, md_len, cs_len);
    return CALMD_OK;
}
