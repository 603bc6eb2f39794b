/*
 * nanosim_amd.h — C ABI of the MI355X-native read-generation engine.
 *
 * The reference (bcgsc/NanoSim v3.2.2, src/simulator.py) has NO FFI/plugin interface: its hot path is
 * a set of module-level Python functions that share ~30 globals filled by read_profile()
 * (src/simulator.py:244-591) and are entered through the mp.Process worker targets
 * (src/simulator.py:1601-1619, 1657-1660).  This header defines the boundary a maintainer would bind
 * at exactly that worker seam; each entry point cites what it replaces.
 *
 * Conventions: plain C, fixed-width little-endian integers, no exceptions across the ABI, every
 * function returns 0 on success or a negative NS_E* code (message via ns_last_error).  The CALLER owns
 * host buffers; the LIBRARY owns device buffers.  One context per GPU, used from one host thread.
 */
#ifndef NANOSIM_AMD_H
#define NANOSIM_AMD_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NS_ABI_VERSION 7u

/* error codes */
#define NS_OK 0
#define NS_EINVAL (-1)   /* bad argument / inconsistent tables */
#define NS_ENODEV (-2)   /* no HIP device / wrong architecture */
#define NS_ENOMEM (-3)   /* device or host allocation failed */
#define NS_EHIP (-4)     /* HIP runtime error (see ns_last_error) */
#define NS_ESTATE (-5)   /* call order violated (no model / no reference / no batch) */
#define NS_EIO (-6)      /* a file write of an output sink failed (ENOSPC, EBADF ...; see ns_last_error) */
#define NS_ESTEP_UNALIGNED (-7) /* ns_generate_step (ABI 7): only the UNALIGNED worker call failed, with an error of its own (anything but
                                 * NS_EHIP, which is returned as such); the aligned batch in info[0] is complete and usable, the cause
                                 * is in ns_last_error */

/* ---- model tables: the flat form of the globals read_profile() fills (src/simulator.py:247-251) ---- */

/* One KDE (sklearn KernelDensity, gaussian): training vector + bandwidth.
 * Replaces kde.sample() at src/simulator.py:235 (i = floor(U*n); x = N(data[i], bw)). */
typedef struct ns_kde {
    const double *data;
    uint64_t n;
    double bw;
} ns_kde;

enum { NS_KDE_ALIGNED = 0,  /* _aligned_region.pkl (or _aligned_reads.pkl with --perfect), S:560,567 */
       NS_KDE_HT = 1,       /* _ht_length.pkl, log10(len+1), S:552 */
       NS_KDE_RATIO = 2,    /* _ht_ratio.pkl, S:555 */
       NS_KDE_UNALIGNED = 3,/* _unaligned_length.pkl, S:545 */
       NS_KDE_GAP = 4,      /* _gap_length.pkl, log10(len+1), S:577 */
       NS_KDE_COUNT = 5 };

/* error types / Markov states (trans_error_pr rows, src/simulator.py:486-495) */
enum { NS_MIS = 0, NS_INS = 1, NS_DEL = 2 };
enum { NS_ST_START = 0, NS_ST_MIS = 1, NS_ST_INS = 2, NS_ST_DEL = 3, NS_ST_MIS0 = 4, NS_ST_INS0 = 5, NS_ST_DEL0 = 6 };

/* quality classes (lognorm_base_qual keys, src/simulator.py:580-591) */
enum { NS_Q_MATCH = 0, NS_Q_MIS = 1, NS_Q_INS = 2, NS_Q_HT = 3, NS_Q_UNMAPPED = 4, NS_Q_COUNT = 5 };
#define NS_QUAL_LEVELS 128u
#define NS_HP_MAX_BREAKS 4u

typedef struct ns_hp_class {          /* one row (AT or CG) of _hp_lengths_model_parameters.tsv */
    double konst, alpha1;             /* predict_piecewise, src/model_homopolymer_lengths.py:167-186 */
    uint32_t n_breaks, _pad;
    double beta[NS_HP_MAX_BREAKS], breakpoint[NS_HP_MAX_BREAKS];
    double intercept, slope;          /* predict_lr, src/model_homopolymer_lengths.py:204-209 */
} ns_hp_class;

typedef struct ns_model_tables {
    uint32_t abi_version;             /* = NS_ABI_VERSION */
    uint32_t flags;                   /* NS_MODEL_* */

    /* ECDF of the first match length: read_ecdf(_first_match.hist), src/simulator.py:194-231,497-498.
     * Segment s covers (hi[s-1], hi[s]] (hi[-1] = 0) and maps linearly onto (vhi[s-1], vhi[s]),
     * vhi[-1] = fm_vlo0. */
    uint32_t fm_nseg, _pad0;
    const double *fm_hi, *fm_vhi;
    double fm_vlo0;

    /* match Markov model: read_ecdf(_match_markov_model), S:500-501; bins of previous match length */
    uint32_t mm_nbins, _pad1;
    const int64_t *mm_bin_lo, *mm_bin_hi;   /* [mm_nbins]  lo <= prev_match < hi, S:1891-1893 */
    const uint32_t *mm_seg_off;             /* [mm_nbins+1] offsets into mm_hi/mm_vhi */
    const double *mm_hi, *mm_vhi;
    const double *mm_vlo0;                  /* [mm_nbins] */

    /* error Markov model rows start,mis,ins,del,mis0,ins0,del0 (S:486-495):
     * trans[s][0] = a (mis is [0,a)), trans[s][1] = a+b (ins is [a,a+b)), trans[s][2] = 1-c (del is [1-c,1)) */
    double trans[7][3];

    /* run-length mixtures (error_par, S:473-484; samplers src/mixed_model.py:41-63) as inverse-CDF tables.
     * mix_cdf[t][0] = first component  (mis: Poisson(lambda)+1;  ins/del: ceil(lambda*Weibull(k)) with 0->1)
     * mix_cdf[t][1] = second component (mis: Geometric(p);       ins/del: Geometric(p)-1 with 0->1)
     * cdf[j] = P(value <= j+1); value = 1 + #{j : p > cdf[j]}, capped at mix_n. */
    double mix_w[3];
    uint32_t mix_n[3][2];
    const double *mix_cdf[3][2];

    ns_kde kde[NS_KDE_COUNT];

    double strandness_rate;           /* _strandness_rate or -s, S:270-275 */
    /* chimeric (S:571-577): number of segments ~ Geometric(1/segment_mean), table as above */
    uint32_t nseg_n, _pad2;
    const double *nseg_cdf;

    /* base qualities (src/model_base_qualities.py:9-20,120-130): per class, thr[j] = round(65536*P(q<=j));
     * q = #{j in [0,126] : h >= thr[j]} for a 16-bit draw h.
     * Contract: each class's thr[0..126] is non-decreasing (ns_load_model returns NS_EINVAL otherwise, naming the class and the
     * level); thr[127] is never read.  Any such table is exact as given: no snapping of thresholds to 64-value buckets is needed.
     * Entries of 65536 or more are never reached by h (<= 65535). */
    uint32_t qual_thr[NS_Q_COUNT][NS_QUAL_LEVELS];

    /* homopolymers (S:504-529; src/model_homopolymer_lengths.py:246-260) */
    ns_hp_class hp[2];                /* 0 = AT, 1 = CG */
    double hp_mis_rate;

    /* transcriptome: the 2-D KDE of (transcript length, aligned length) (_aligned_region_2d.pkl, S:561-565), training points sorted
     * by transcript length; select_nearest_kde2d (S:108-111) becomes a draw from the KDE conditioned on the transcript length */
    const double *kde2d_x, *kde2d_y;
    uint64_t kde2d_n;
    double kde2d_bw;
} ns_model_tables;

#define NS_MODEL_HAS_ERRORS 1u   /* error tables present (absent with --perfect) */
#define NS_MODEL_HAS_QUALS 2u
#define NS_MODEL_HAS_HP 4u
#define NS_MODEL_HAS_CHIMERIC 8u
#define NS_MODEL_HAS_UNALIGNED 16u
#define NS_MODEL_HAS_KDE2D 32u

/* ---- generation parameters: the arguments of the worker targets ------------------------------------
 * simulation_aligned_genome(dna_type, min_l, max_l, median_l, sd_l, out_reads, out_error, kmer_bias,
 *                           fastq, num_simulate, per, chimeric)            src/simulator.py:1266-1267
 * simulation_unaligned(dna_type, min_l, max_l, median_l, sd_l, out_reads, fastq, num_simulate, uracil)
 *                                                                          src/simulator.py:1482      */
enum { NS_KIND_ALIGNED = 0, NS_KIND_UNALIGNED = 1, NS_KIND_PERFECT = 2 };
#define NS_EMIT_SIZES 2u

typedef struct ns_params {
    uint64_t seed;          /* Philox key; (seed, read index) fully determine a read */
    uint64_t first_read;    /* global index of the first read of this batch (also the number in the name) */
    uint64_t n_reads;       /* num_simulate for this call */
    uint32_t kind;          /* NS_KIND_* */
    uint32_t fastq;         /* emit qualities / FASTQ records */
    uint32_t kmer_bias;     /* k of -k/--KmerBias; 0 = off (falsy in the reference, S:1413,1920) */
    uint32_t chimeric;
    uint32_t use_lognormal; /* -med/-sd given */
    uint32_t emit_records;  /* 1: format FASTA/FASTQ records on the device; NS_EMIT_SIZES: compute record_bytes / errlog_bytes of the batch
                             * without writing the images (sizing pass of a multi-rank run: every rank then writes at its final file offset) */
    int64_t min_len, max_len;
    double median_len, sd_len;
    uint32_t emit_errlog;   /* 1: format the _aligned_error_profile rows on the device (S:2006-2008); needs emit_records != 0 (the rows
                             * quote the read names of the record image): with emit_records = 0 errlog_bytes is 0 */
    uint32_t meta;          /* 1: metagenome batch = one worker of simulation_aligned_metagenome (S:814-1040) / simulation_unaligned("metagenome") */
    uint32_t trx;           /* 1: transcriptome batch = one worker of simulation_aligned_transcriptome (S:1043-1263) /
                             * simulation_unaligned("transcriptome"); needs ns_set_transcriptome */
    uint32_t uracil;        /* --uracil: T -> U in the emitted sequence (S:1247-1248) */
    uint32_t model_ir;      /* transcriptome, aligned reads: intron retention (S:1156-1183); needs ns_set_intron_retention */
    uint32_t reserved0;
} ns_params;

/* ---- device-side result layout (copied out with ns_copy_out) -------------------------------------- */

/* one e_dict entry (S:1875-1882), ascending order, position in un-mutated segment coordinates.
 * info = len[0:12] | type[12:14] | (shift + 2^17)[14:32]; shift = sum(ins - del) over the earlier events of
 * the same piece, so the payload of the event starts at emitted-segment offset pos + shift.  An attempt of a read with an event
 * outside these fields (multi-megabase reads only) is dropped and the read redrawn: ns_batch_info.n_range_redraws. */
typedef struct ns_event {
    uint32_t pos;           /* ceil(key): mis/del at pos, ins before index pos */
    uint32_t info;
} ns_event;
#define NS_EV_LEN_MAX 4095u
#define NS_EV_SHIFT_BIAS 131072
#define NS_EV_LEN(info) ((uint32_t)(info) & 0xfffu)
#define NS_EV_TYPE(info) (((uint32_t)(info) >> 12) & 3u)
#define NS_EV_SHIFT(info) ((int32_t)((uint32_t)(info) >> 14) - NS_EV_SHIFT_BIAS)
#define NS_EV_PACK(len, type, shift) (((uint32_t)(len) & 0xfffu) | ((uint32_t)(type) & 3u) << 12 | (uint32_t)((shift) + NS_EV_SHIFT_BIAS) << 14)

typedef struct ns_piece {   /* one aligned segment or one chimeric gap / unaligned body */
    uint64_t ref_gpos;      /* start offset in the concatenated reference; >= NS_SPLICED_BASE: offset of a spliced pre-mRNA
                             * stretch (intron retention) in the batch's splice arena (NS_BUF_SPLICED) */
    uint64_t ev_off;        /* first event in the event buffer */
    uint32_t chrom;
    uint32_t pos;           /* start inside the chromosome (the number in the read name, S:1747,1778) */
    uint32_t ref_len;       /* middle_ref: reference bases consumed (S:1363) */
    uint32_t out_len;       /* bases emitted for this piece */
    uint32_t n_ev;
    uint32_t kind;          /* 0 aligned segment, 1 gap / unaligned */
} ns_piece;

typedef struct ns_read {
    uint64_t rec_off;       /* byte offset of the record in the record buffer */
    uint32_t piece_off;     /* first piece */
    uint16_t n_pieces;      /* 2*segments-1 */
    uint8_t reversed;       /* is_reversed, S:1312 */
    uint8_t flags;
    uint32_t head, tail;    /* S:1377-1382 */
    uint32_t seq_len;       /* emitted bases incl. head/tail */
    uint32_t attempts;      /* rejected attempts before this one (S:1367) */
} ns_read;

typedef struct ns_batch_info {
    uint64_t n_reads, n_pieces;
    uint64_t n_events;      /* length of the event buffer (pieces index it through ev_off; capacity gaps included) */
    uint64_t events_used;   /* events actually generated */
    uint64_t record_bytes;  /* size of the FASTA/FASTQ image */
    uint64_t errlog_bytes;  /* size of the error-profile image */
    uint64_t total_bases;   /* sum of seq_len */
    uint64_t total_ref_bases; /* sum of ref_len over pieces (for the roofline byte count) */
    uint64_t n_overflow;    /* reads that needed the event-capacity fallback pass */
    double ms_total;        /* device time of the whole batch (HIP events on the engine stream) */
    double ms_kernel[8];    /* per-kernel device time: see NS_K_* */
    uint64_t spliced_bytes; /* intron retention: size of the splice arena (NS_BUF_SPLICED) */
    uint64_t n_range_redraws; /* attempts dropped because an event did not fit the 8-byte record (NS_EV_LEN_MAX / the shift field): the
                               * read drew new lengths, as after a failed final length check (S:1429-1430) */
} ns_batch_info;

enum { NS_K_LENGTHS = 0, NS_K_EVENTS = 1, NS_K_SCAN = 2, NS_K_MATERIALISE = 3, NS_K_HP = 4, NS_K_ERRLOG = 5,
       NS_K_RECORD_KERNEL = 6 };   /* 6: the record kernel alone (k_materialise; with -k: its last pass) — NS_K_MATERIALISE is the record STAGE:
                                    * that kernel, the generic kernel for the tiles it queued, the quality lines, the join with k_names */
enum { NS_BUF_RECORDS = 0, NS_BUF_READS = 1, NS_BUF_PIECES = 2, NS_BUF_EVENTS = 3, NS_BUF_ERRLOG = 4,
       NS_BUF_POLYA = 5 /* uint16 per read: polyA tail length of a transcriptome batch */,
       NS_BUF_SPLICED = 6 /* intron retention: the spliced stretches (transcript orientation, device form of the bases) */ };

typedef struct ns_ctx ns_ctx;

/* lifecycle */
int ns_create(int device, ns_ctx **out);
void ns_destroy(ns_ctx *ctx);
const char *ns_last_error(const ns_ctx *ctx);
uint32_t ns_abi_version(void);
/* A context whose worker calls run NEXT TO another context's on the same GPU (the reference runs its workers side by side, -t,
 * S:1588-1605; the unaligned worker call of a step runs like that).  A scheduling hint only — the reads are the same either way.
 * Until ABI 6 / round 5 it sent all but the longest eighth of a batch of unaligned reads through the thread-per-read error list;
 * since round 6 every unaligned read takes the wave-per-read one on either kind of context (NS_UCOOP_SHIFT=3 restores the split). */
int ns_set_background(ns_ctx *ctx, int on);

/* reference genome: replaces seq_dict/seq_len/genome_len (src/simulator.py:279-353).  `bases` is the
 * concatenation of all chromosomes as read from the FASTA (any case, IUPAC allowed); chrom_off has
 * nchrom+1 entries; circular[i] != 0 marks a circular chromosome (-dna_type circular, dict_dna_type);
 * names is a NUL-separated blob of the (already normalised, S:344-347) chromosome names. */
int ns_set_reference(ns_ctx *ctx, const uint8_t *bases, uint64_t nbases, const uint64_t *chrom_off,
                     uint32_t nchrom, const uint8_t *circular, const char *names, uint64_t names_len);
/* same, but `bases_dev` is already resident in this GPU's HBM (e.g. filled by an RCCL broadcast): the library makes a
 * device-to-device copy (normalised, padded for its unaligned loads); the caller's buffer is neither modified nor kept. */
int ns_set_reference_device(ns_ctx *ctx, const void *bases_dev, uint64_t nbases, const uint64_t *chrom_off,
                            uint32_t nchrom, const uint8_t *circular, const char *names, uint64_t names_len);

/* metagenome (src/simulator.py:284-339, 357-380): chromosomes of species s are [species_chrom_off[s], species_chrom_off[s+1]) of
 * the reference set with ns_set_reference (chromosome names are then "<species>-<chrom>", S:1747); abun = dict_abun of the
 * sample, abun_inflated = dict_abun_inflated (NULL unless chimeric, S:2511-2514).  ns_species_bases returns
 * current_species_bases (S:835, 1001-1002) of the last metagenome batch. */
int ns_set_species(ns_ctx *ctx, uint32_t nspecies, const uint32_t *species_chrom_off);
int ns_set_abundance(ns_ctx *ctx, const double *abun, const double *abun_inflated);
int ns_species_bases(ns_ctx *ctx, double *out);

/* transcriptome (src/simulator.py:341-350, 382-399, 460-470): the transcripts are the "chromosomes" of the reference set with
 * ns_set_reference (all linear).  expr_chrom / expr_cum: the transcripts with TPM > 0 in the order of make_cdf (S:69-97, ascending
 * expression) and the cumulative weights random.choices builds from ecdf_weight_list (S:1084); polya[nchrom] != 0 marks the
 * transcripts of the --polya list (NULL: none); polya_scale = scale of the exponential tail length (S:1046-1053). */
int ns_set_transcriptome(ns_ctx *ctx, uint32_t n_expr, const uint32_t *expr_chrom, const double *expr_cum,
                         const uint8_t *polya, double polya_scale);

/* intron retention (src/simulator.py:403-452: the GFF3 structure of the transcripts, the IR Markov model and the genome FASTA
 * that pysam serves in the reference).  Items of transcript t (a chromosome of the reference set with ns_set_reference) are
 * item_off[t] .. item_off[t+1]-1 in GFF3 order; coordinates are HTSeq's (0-based start, length = end - start).  A read of a
 * transcript in which update_structure (S:114-145) flags at least one intron as retained is cut from the genome by
 * extract_read_pos (S:148-191, 1159-1177): its piece has pos = the genome coordinate in the read name and
 * ref_gpos >= NS_SPLICED_BASE.  The host arrays are copied; NULL switches the feature off. */
typedef struct ns_ir_tables {
    const uint8_t *genome;          /* bases of the genome FASTA as they are in the file (case matters: S:1675-1680) */
    const uint64_t *genome_off;     /* [n_gchrom + 1] */
    uint32_t n_gchrom;
    uint32_t n_items;
    const uint32_t *item_off;       /* [n transcripts + 1] */
    const uint8_t *item_type;       /* NS_IR_EXON / NS_IR_INTRON */
    const uint8_t *item_minus;      /* 1: strand '-' */
    const uint32_t *item_chrom;     /* chromosome of the genome FASTA; NS_IR_NO_CHROM: not in the file (S:1167-1169) */
    const uint32_t *item_start;
    const uint32_t *item_len;
    double p_no_ir[3], p_ir[3];     /* rows start / no_IR / IR of <prefix>_IR_markov_model (S:414-422) */
} ns_ir_tables;
enum { NS_IR_EXON = 0, NS_IR_INTRON = 1 };
#define NS_IR_NO_CHROM 0xffffffffu
#define NS_SPLICED_BASE (1ull << 56)
int ns_set_intron_retention(ns_ctx *ctx, const ns_ir_tables *tables);

/* model: replaces the globals filled by read_profile() (src/simulator.py:473-591) */
int ns_load_model(ns_ctx *ctx, const ns_model_tables *tables);

/* the hot path: replaces one worker call simulation_aligned_genome / simulation_unaligned
 * (src/simulator.py:1266-1454, 1482-1549).  Results stay in HBM until the next ns_generate; the record and error-profile images
 * live in one of TWO result slots, so that a batch queued with ns_sink_write leaves the device while the next one is generated. */
int ns_generate(ns_ctx *ctx, const ns_params *params, ns_batch_info *info);

/* One STEP of simulation() (src/simulator.py:1571-1672): the aligned worker call (S:1601-1619 -> simulation_aligned_*) and the unaligned
 * one (S:1657-1660 -> simulation_unaligned) of the same share of the run, side by side on this GPU.  The reference joins the aligned
 * workers before it starts the unaligned ones (S:1621-1622); that order constrains the FILES only — the two calls write different files
 * and a read is a function of (seed, read index) — so the library runs them next to each other: the aligned call on `ctx`, the unaligned
 * one on the context's STEP COMPANION (own streams and batch buffers on the same device; it shares the reference, the model and the
 * mode tables of `ctx` — nothing is uploaded twice) from a worker thread the library keeps.  info[0] = the aligned batch, info[1] = the unaligned one; either params
 * pointer may be NULL (that call is skipped and its info zeroed).  The bytes of both batches are those of two ns_generate calls.
 * The unaligned batch's buffers belong to the companion: ns_step_context returns it (created on first use, owned and destroyed by
 * `ctx`; never pass it to ns_destroy) for ns_copy_out / ns_device_ptr / ns_record_offsets / ns_sink_* / ns_io_counters.
 * Errors: a failed aligned call returns its own code.  A failed unaligned call returns NS_ESTEP_UNALIGNED (ABI 7) — also when
 * `aligned` is NULL — and info[0] then holds the complete aligned batch (if one was asked for); the unaligned call's own code (NS_EINVAL,
 * NS_ESTATE, NS_ENOMEM, NS_EIO) is in the ns_last_error text: "unaligned worker call (error <code>): ...".  An NS_EHIP of the unaligned
 * call is returned unchanged (a HIP error can leave the device unusable for both calls).
 * Added with ABI 6; ns_generate is unchanged. */
int ns_generate_step(ns_ctx *ctx, const ns_params *aligned, const ns_params *unaligned, ns_batch_info info[2]);
int ns_step_context(ns_ctx *ctx, ns_ctx **companion);

/* copy a result buffer of the last batch to host memory; nbytes must not exceed the buffer size
 * (record_bytes, n_reads*sizeof(ns_read), n_pieces*sizeof(ns_piece), n_events*sizeof(ns_event), errlog_bytes) */
int ns_copy_out(ns_ctx *ctx, int which, void *host_dst, uint64_t offset, uint64_t nbytes);
/* page-locked host memory for ns_copy_out destinations (the worker's out_reads / out_error writes, src/simulator.py:1437-1443,
 * 2006-2008, become DMA transfers at PCIe rate into such a buffer followed by plain file writes).  Owned by the caller. */
int ns_host_alloc(ns_ctx *ctx, uint64_t nbytes, void **out);
int ns_host_free(ns_ctx *ctx, void *p);

/* ---- output sinks: the worker's out_reads.write(...) / out_error.write(...) (src/simulator.py:1437-1443, 2006-2008) ----------------
 * A sink is an open file (descriptor owned by the caller) that the library appends result buffers to: ns_sink_write queues the record
 * image (NS_BUF_RECORDS) or the error-profile image (NS_BUF_ERRLOG) of the LAST batch and returns at once.  The bytes travel in
 * slices over the context's copy stream (DMA, concurrent with the kernels of the next ns_generate) into page-locked staging memory
 * and from there to the file with pwrite() at their final offsets, on the library's writer threads.  The next ns_generate fills the
 * other result slot; the one after it waits until the queued copies have left the device.  fd < 0: the bytes are copied to the host
 * and dropped.  ns_sink_put appends host bytes (the header line of the error profile, S:1634) in order with the queued buffers.
 * ns_sink_drain waits until everything queued is in the file and reports the first write error (NS_EIO); file_off (optional)
 * receives the offset behind the last byte.  Tuning (environment, read by the first ns_sink_open of a context): NS_IO_SLICE_MB
 * (16), NS_IO_SLICES (24), NS_IO_THREADS (16; at most one of them writes into a given file at a time). */
typedef struct ns_sink ns_sink;
int ns_sink_open(ns_ctx *ctx, int fd, uint64_t file_off, ns_sink **out);
int ns_sink_put(ns_ctx *ctx, ns_sink *sink, const void *host_src, uint64_t nbytes);
int ns_sink_write(ns_ctx *ctx, ns_sink *sink, int which);
/* the same for bytes [offset, offset + nbytes) of the buffer: one batch spread over several files (the reference's workers write
 * sub-files that are concatenated afterwards, S:1588-1639; several inodes are what lets the file writes run in parallel).
 * ns_record_offsets gives the cut points: for read indices of the last batch (0 .. n_reads; n_reads = the end) the byte offset of
 * the read's record in the record image and of its first row in the error-profile image (err_off may be NULL). */
int ns_sink_write_range(ns_ctx *ctx, ns_sink *sink, int which, uint64_t offset, uint64_t nbytes);
int ns_record_offsets(ns_ctx *ctx, const uint64_t *read_index, uint32_t n, uint64_t *rec_off, uint64_t *err_off);
int ns_sink_drain(ns_ctx *ctx, ns_sink *sink, uint64_t *file_off);
int ns_sink_close(ns_ctx *ctx, ns_sink *sink);
typedef struct ns_io_stats {
    uint64_t bytes;          /* bytes copied device -> host through the sinks of this context */
    double dma_ms;           /* sum of the slices' copy durations (HIP events on the copy stream): bytes / dma_ms = the DMA rate */
    double wait_staging_s;   /* time the copier waited for a free staging slice (the file writes are the limit when this is large) */
    double write_s;          /* sum of the writer threads' time in pwrite() */
    uint64_t slice_bytes;
    uint32_t n_slices, n_threads;
} ns_io_stats;
int ns_io_counters(ns_ctx *ctx, ns_io_stats *out, int reset);

/* ---- training side: the histograms of the characterisation stage ---------------------------------------------------------------------
 * replaces the counting loop of src/besthit_to_histogram.py:hist() (B:316-365 over parse_cs, B:41-69): from the cs strings of the primary
 * alignments (minimap2's short form: `:N` match, `*xy` mismatch, `+seq` insertion, `-seq` deletion) to
 *   dic[0..4]    run-length histograms of add_dict (B:14-22; values above 1000 are not counted): matches between errors, the first
 *                match of every alignment, mismatch runs, insertions, deletions           -> _match.hist, _first_match.hist, _mis/_ins/_del.hist
 *   match_list   (previous match, next match) counts of add_match (B:25-38; no upper limit) -> _match_markov_model
 *   error_list   error transitions, row = mis, ins, del, mis0, ins0, del0 (the previous error, "0": no match in between), column = mis,
 *                ins, del; first_error: the first error of every alignment                   -> _error_markov_model
 * cs: the strings back to back, aln_off[n_aln + 1] their offsets (host memory; copied to the device).  The tables the reference writes
 * from these counts are text formatting on the host (nanosim_amd/characterize/errors.py).  match_list is a dense cap x cap matrix in caller-owned
 * host memory: an add_match with an index >= cap is counted in n_match2d_overflow and max_match says how large the matrix has to be. */
typedef struct ns_cs_hist {
    uint32_t cap_match2d;         /* in */
    uint32_t _pad;
    uint64_t *match_list;         /* in: host buffer of cap_match2d * cap_match2d counters (row = previous match length), or NULL */
    uint64_t dic[5][1001];        /* out: NS_CSH_MATCH, NS_CSH_FIRST_MATCH, NS_CSH_MIS, NS_CSH_INS, NS_CSH_DEL */
    uint64_t error_list[18];
    uint64_t first_error[3];
    uint64_t max_match;           /* largest length handed to add_match */
    uint64_t n_match2d_overflow;
    uint64_t n_skip;              /* `=` items (long-form cs): the reference's two lists fall out of step on them — refuse the input */
    double ms_kernel;
} ns_cs_hist;
enum { NS_CSH_MATCH = 0, NS_CSH_FIRST_MATCH = 1, NS_CSH_MIS = 2, NS_CSH_INS = 3, NS_CSH_DEL = 4 };
int ns_cs_histograms(ns_ctx *ctx, const uint8_t *cs, uint64_t nbytes, const uint64_t *aln_off, uint32_t n_aln, ns_cs_hist *h);
/* The MAF branch of the same loop (B:188-315): <prefix>_besthit.maf carries two `s` lines per alignment, the aligned reference and query
 * sequences with '-' for gaps.  ref_lines / query_lines: those lines (field 7) of all alignments back to back, alignment a at
 * aln_off[a] .. aln_off[a + 1] of BOTH (the two lines of an alignment have the same length; nbytes = aln_off[n_aln]).  Same counters,
 * same struct; per alignment the state of the reference's column walk (its four pending run lengths, prev_match and prev_error reset
 * per alignment).  Added with ABI 6. */
int ns_maf_histograms(ns_ctx *ctx, const uint8_t *ref_lines, const uint8_t *query_lines, uint64_t nbytes, const uint64_t *aln_off,
                      uint32_t n_aln, ns_cs_hist *h);

/* ---- training side: the base-quality model ---------------------------------------------------------------------------------------------
 * replaces the collecting loops of src/model_base_qualities.py (M:23-79): for every query base of every primary alignment its class —
 * mismatch, insertion, match (from the cs string), head / tail (the soft clips), unmapped (every base of an unmapped read) — and its
 * quality, as a histogram per class.  The log-normal fit the reference runs on the collected values (M:82-96) is a closed form of the
 * histogram and is done on the host (nanosim_amd/characterize/qualities.py: fit_qualities).
 * cs / qual: the cs strings and the QUAL strings (SAM text, Phred + 33; soft clips included, hard clips are not in QUAL) of the
 * alignments back to back in host memory, alignment a at cs_off[a] .. cs_off[a + 1] and qual_off[a] .. qual_off[a + 1]; aln[a]: its soft
 * clips.  head + tail must not exceed the alignment's quality length.  Added without an ABI change (a new function breaks no caller). */
typedef struct ns_qual_aln { uint32_t head, tail, unmapped, reserved; } ns_qual_aln;   /* soft-clip lengths in bases; unmapped != 0: whole string is class 4, cs ignored */
typedef struct ns_qual_hist {
    uint64_t hist[5][128];      /* [mis, ins, match, ht, unmapped][quality 0..93]; the rest stays 0 */
    uint64_t n_short;           /* alignments whose cs covers fewer bases than qual_len - head - tail */
    uint64_t n_bad_qual;        /* bytes outside '!'..'~' (not counted anywhere else) */
    double   ms_kernel;
} ns_qual_hist;
enum { NS_QH_MIS = 0, NS_QH_INS = 1, NS_QH_MATCH = 2, NS_QH_HT = 3, NS_QH_UNMAPPED = 4 };
int ns_qual_histograms(ns_ctx *ctx, const uint8_t *cs, uint64_t cs_bytes, const uint64_t *cs_off,
                       const uint8_t *qual, uint64_t qual_bytes, const uint64_t *qual_off,
                       const ns_qual_aln *aln, uint32_t n_aln, ns_qual_hist *out);

/* ---- training side: the homopolymer-length model ---------------------------------------------------------------------------------------
 * replaces the per-alignment loop of src/model_homopolymer_lengths.py (analyze_homopolymers H:64-119, calc_homopolymer_mis_rate H:9-33):
 * for every homopolymer of the reference line with at least min_hp_len (>= 1) letters its length there and the length the read shows
 * for it (the reference's fuzzy regular expression, restated in nanosim_amd/csrc/ns_hp_hist.h), counted per class — AT, CG — in
 *   table[2][cap_ref][cap_read]   dense, in caller-owned host memory (row = reference length, column = read length); a homopolymer with
 *                                 ref_len >= cap_ref or read_len >= cap_read counts in n_overflow, and max_ref / max_read (the largest
 *                                 lengths met) say how large the table has to be;
 *   columns[4]                    insertions, deletions, mismatches, matches over the columns of all homopolymer spans (H:15-31);
 *   records                       optional (NULL: none): one ns_hp_record per homopolymer, alignment by alignment in the order of the
 *                                 call and left to right inside an alignment.  n_hp is their number; when it exceeds cap_records none
 *                                 is written: call again with a larger buffer.
 * The fits the reference runs on these (H:142-201) are done on the host (nanosim_amd/characterize/homopolymers.py: fit_homopolymers).
 * ref_lines / query_lines / aln_off: as ns_maf_histograms; an alignment may have at most 2^24 - 1 columns.  Added without an ABI change. */
typedef struct ns_hp_record {
    uint32_t aln;               /* index of the alignment in the call */
    uint32_t start;             /* first letter of the homopolymer in the dash-less reference line */
    uint32_t ref_len;
    uint32_t read_base;         /* read_len << 2 | base (0 A, 1 C, 2 G, 3 T) */
} ns_hp_record;
typedef struct ns_hp_hist {
    uint32_t cap_ref, cap_read;   /* in: 1 .. 65536 each, cap_ref * cap_read <= 2^26 */
    uint64_t *table;              /* in: host buffer of 2 * cap_ref * cap_read counters */
    ns_hp_record *records;        /* in: host buffer of cap_records records, or NULL */
    uint64_t cap_records;         /* in */
    uint64_t n_hp;                /* out: homopolymers (inside the table or not) */
    uint64_t columns[4];          /* out: NS_HPC_INS, NS_HPC_DEL, NS_HPC_MIS, NS_HPC_MATCH */
    uint64_t max_ref, max_read;
    uint64_t n_overflow;
    double ms_kernel;
} ns_hp_hist;
enum { NS_HPC_INS = 0, NS_HPC_DEL = 1, NS_HPC_MIS = 2, NS_HPC_MATCH = 3 };
int ns_hp_histograms(ns_ctx *ctx, const uint8_t *ref_lines, const uint8_t *query_lines, uint64_t nbytes, const uint64_t *aln_off,
                     uint32_t n_aln, uint32_t min_hp_len, ns_hp_hist *out);

/* ---- training side: aligned line pairs from SAM records -----------------------------------------------------------------------------------
 * replaces `samtools view | sam2pairwise` + src/pairwise2maf.py:38-82 (src/read_analysis.py:200-204): per record, from its CIGAR, its
 * MD:Z tag and its SEQ (as SAM holds it), the aligned reference line and the aligned read line with `-` for gaps — the M/=/X/I/D columns
 * only, clips cut — and its four figures.  Strings lie back to back with one table of n_aln + 1 offsets each, as in ns_qual_histograms.
 * What makes a record BAD is listed in nanosim_amd/csrc/ns_sam_pairs.h: it gets zero columns and all-zero figures, is counted in n_bad,
 * and first_bad is the index of the first one (n_aln when there is none).
 * aln_off, aln (unless NULL), n_bytes and the bad counters are always written.  The lines are written only when buffers are given and
 * n_bytes <= cap_bytes: size them from a first call with NULL lines.  Added without an ABI change.
 * ns_hp_histograms_sam: the conversion, then ns_hp_histograms on the lines where they are, on the device; `pairs` may be NULL (nothing of
 * the conversion goes back to the host) or carry buffers as above.  With n_bad > 0 nothing is counted (`out` is all zero). */
typedef struct ns_sam_aln { uint32_t head, tail, ref_len, query_len; } ns_sam_aln;
typedef struct ns_sam_pairs {
    uint8_t *ref_lines, *query_lines;  /* in: host buffers of cap_bytes each, or both NULL */
    uint64_t cap_bytes;                /* in */
    uint64_t *aln_off;                 /* in: host buffer of n_aln + 1 offsets (out) */
    ns_sam_aln *aln;                   /* in: host buffer of n_aln entries (out), or NULL */
    uint64_t n_bytes;                  /* out: columns of all records = aln_off[n_aln] */
    uint64_t n_bad, first_bad;         /* out */
    double ms_kernel;
} ns_sam_pairs;
int ns_sam_pairs_build(ns_ctx *ctx, const uint8_t *cigar, const uint64_t *cigar_off, const uint8_t *md, const uint64_t *md_off,
                       const uint8_t *seq, const uint64_t *seq_off, uint32_t n_aln, ns_sam_pairs *out);
int ns_hp_histograms_sam(ns_ctx *ctx, const uint8_t *cigar, const uint64_t *cigar_off, const uint8_t *md, const uint64_t *md_off,
                         const uint8_t *seq, const uint64_t *seq_off, uint32_t n_aln, uint32_t min_hp_len, ns_sam_pairs *pairs,
                         ns_hp_hist *out);

/* ---- training side: the error-length mixtures ------------------------------------------------------------------------------------------------
 * replaces the grid of Nelder-Mead searches of src/model_fitting.py (mis_fit / ins_fit / del_fit, F:59-105, run from F:116-214): one search
 * per start, all of them in one kernel.  cdf[n_bins] is the empirical CDF of the run lengths (read_histogram, F:27-45), 1 .. 65536 bins.
 *   NS_MIXFIT_MISMATCH   3 doubles per start (l, p, w): Poisson-geometric, bins are x = 0 .. n_bins-1 (mis_ll);
 *   NS_MIXFIT_INDEL      4 doubles per start (l, k, p, w): Weibull-geometric, bins are x = 1 .. n_bins (ins_ll, del_ll).
 * The objective is the largest |model CDF - cdf|; it is NaN when a parameter is not > 0 or p > 1 (scipy's argument checks).  The search is
 * scipy's minimize(f, x0, method='Nelder-Mead') with its defaults; objective, evaluation order and search are written down in
 * nanosim_amd/csrc/ns_mixfit.h.  NS_MIXFIT_EVALUATE returns the objective at each given point instead (fun = residual, nfev = 1, nit = 0).
 * Selecting among the starts and writing <prefix>_model_profile is done on the host (nanosim_amd/characterize/mixfit.py: fit_mixtures).
 * Added without an ABI change. */
enum { NS_MIXFIT_MISMATCH = 0, NS_MIXFIT_INDEL = 1 };
enum { NS_MIXFIT_FIT = 0, NS_MIXFIT_EVALUATE = 1 };
typedef struct ns_mixfit_fit {
    double   x[4];              /* the result point sim[0]; entries beyond the kind's parameters are 0 */
    double   fun;               /* scipy's result.fun = np.min(fsim): NaN as soon as one vertex of the last simplex is */
    double   residual;          /* the objective at x (what mis_fit / ins_fit / del_fit return as diff) */
    uint32_t nfev, nit;
    int32_t  status;            /* 0 converged, 1 the evaluation limit, 2 the iteration limit (200 per parameter each) */
    uint32_t reserved;
} ns_mixfit_fit;
typedef struct ns_mixfit_result {
    ns_mixfit_fit *fits;        /* in: host buffer of n_starts entries (out) */
    double ms_kernel;
} ns_mixfit_result;
int ns_mixture_fit(ns_ctx *ctx, int kind, const double *cdf, uint32_t n_bins, const double *starts, uint32_t n_starts, int mode,
                   ns_mixfit_result *out);

/* ---- training side: the lengths behind the read-length models ---------------------------------------------------------------------------------
 * replaces the loop of src/head_align_tail_dist.py (head_align_tail, A:134-229) over the primary alignments: per record, from its CIGAR
 * text, FLAG 0x10, POS and the LN of its reference, what pysam computes for it (ns_len_aln; nanosim_amd/csrc/ns_read_len.h says how, and
 * what makes a record BAD: all figures 0, counted in n_bad, first_bad the smallest index of one, n_aln without); per read — the records
 * read_off[r] .. read_off[r + 1] - 1, at least one — the largest read_len, the smallest head and tail (each also against extra_head /
 * extra_tail of the read when given and not 0xffffffff) and its number of aligned segments; and the aligned segments themselves, in
 * record order: the sum of ref_len over records that the reference joins as the two ends of a circular reference (NS_LEN_GENOME), or
 * one per record (NS_LEN_TRANSCRIPTOME).  edge: bit 0 the alignment lies at the start of its reference, bit 1 at its end.
 * ref_start is POS - 1.  Added without an ABI change. */
typedef struct ns_len_aln  { uint32_t head, tail, read_len, ref_len, query_aln_len, edge; } ns_len_aln;
typedef struct ns_len_read { uint32_t read_len, head, tail, n_segments; } ns_len_read;
typedef struct ns_len_result {
    ns_len_aln *aln;            /* in: host buffer of n_aln entries (out), or NULL */
    ns_len_read *reads;         /* in: host buffer of n_reads entries (out) */
    uint64_t *segments;         /* in: host buffer of n_aln entries; the first n_segments are written */
    uint64_t n_segments;        /* out */
    uint64_t n_bad, first_bad;  /* out */
    double ms_kernel;
} ns_len_result;
#define NS_LEN_GENOME 0
#define NS_LEN_TRANSCRIPTOME 1
int ns_read_lengths(ns_ctx *ctx, const uint8_t *cigar, const uint64_t *cigar_off, const uint8_t *reverse, const uint32_t *ref_id,
                    const uint64_t *ref_start, const uint64_t *ref_total, uint32_t n_refs, const uint64_t *read_off, uint32_t n_reads,
                    uint32_t n_aln, int mode, const uint32_t *extra_head, const uint32_t *extra_tail, ns_len_result *out);

/* ---- training side: chimeric reads, the split-alignment choice ----------------------------------------------------------------------------------
 * replaces the decisions of primary_and_unaligned_chimeric (src/get_primary_sam.py, G:273-395) for every primary alignment and the
 * entries of its SA:Z tag; nanosim_amd/csrc/ns_chimeric.h says how, with every corner of the reference that is kept.
 * ns_cigar_spans: per CIGAR text what cigar_parser (G:16-31) gives — qstart, qend, qlen = M + I, rlen = M + D.  A BAD CIGAR has all
 * figures 0, is counted in *n_bad, *first_bad the smallest index of one (n without).  The caller also runs it over the CIGARs of the
 * file's supplementary and secondary records, which the reference matches to the chosen pieces by these figures (G:397-402).
 * ns_chimeric_select: the reads r = 0 .. n_reads - 1 have the entries ent_off[r] .. ent_off[r + 1] - 1, at least one: the first is the
 * primary alignment (its figures are pysam's: qstart = leading S, qlen = M + I + `=` + X, rlen = M + D + N + `=` + X), the others the SA
 * entries in tag order.  Per entry: its CIGAR, ref_id (< n_refs), ref_start (0-based), nm, reverse (direction is not `+`); per reference
 * ref_total (LN) and species (< n_species).  Out: ent[n_ent] the figures (optional), reads[n_reads], pieces[n_ent] — the pieces of read
 * r in query order from pieces[ent_off[r]] on, reads[r].n_pieces of them: the entry's index inside the read, whether the reference takes
 * it for the primary record (its qstart is the primary's), and the gap in front of it or NS_CHIM_NO_GAP —, species_count[n_species][2]
 * (the gaps behind a piece of the species: [0] the next piece is of the same species, [1] of another), n_gaps, pos_strand.
 * With a bad CIGAR (n_bad != 0) everything else is undefined.  Added without an ABI change. */
typedef struct ns_chim_ent   { uint32_t qstart, qend, qlen, rlen; } ns_chim_ent;
typedef struct ns_chim_piece { uint32_t entry, is_primary; int64_t gap; } ns_chim_piece;
typedef struct ns_chim_read  { uint32_t n_pieces, flags; } ns_chim_read;
#define NS_CHIM_NO_GAP (-1)
#define NS_CHIM_POS_STRAND 1u      /* ns_chim_read.flags: the read adds to pos_strand */
#define NS_CHIM_ALONE 2u           /* the winning list was one piece that is not the primary: the primary record is kept alone */
#define NS_CHIM_HAS_SA 4u          /* the read has SA entries */
typedef struct ns_chim_result {
    ns_chim_ent *ent;           /* in: host buffer of n_ent entries (out), or NULL */
    ns_chim_piece *pieces;      /* in: host buffer of n_ent entries (out) */
    ns_chim_read *reads;        /* in: host buffer of n_reads entries (out) */
    uint64_t *species_count;    /* in: host buffer of n_species * 2 entries (out) */
    uint64_t n_gaps, pos_strand;/* out */
    uint64_t n_bad, first_bad;  /* out */
    double ms_kernel;           /* both kernels */
    double ms_scan;             /* k_chim_scan (with the visiting order) alone */
} ns_chim_result;
int ns_cigar_spans(ns_ctx *ctx, const uint8_t *cigar, const uint64_t *cigar_off, uint32_t n, ns_chim_ent *out, uint64_t *n_bad,
                   uint64_t *first_bad, double *ms_kernel);
int ns_chimeric_select(ns_ctx *ctx, const uint8_t *cigar, const uint64_t *cigar_off, const uint64_t *ent_off, uint32_t n_reads,
                       const uint32_t *ref_id, const uint64_t *ref_start, const uint32_t *nm, const uint8_t *reverse,
                       const uint64_t *ref_total, const uint32_t *species, uint32_t n_refs, uint32_t n_species, ns_chim_result *out);

/* ---- training side: abundance quantification, the EM over multi-mapping reads --------------------------------------------------------------------
 * replaces the loops of EM_meta and EM_trans (src/get_primary_sam.py, G:60-84, G:104-127); nanosim_amd/csrc/ns_em.h says how: every sum in
 * the reference's order, so that abundance, count, the diff of every iteration and the iteration on which the loop ends are the
 * reference's bit for bit.  The targets t = 0 .. n_targets - 1 are the species (meta) or transcripts (trans) in the order of the @SQ-derived
 * dict; the items m = 0 .. n_multi - 1 are the entries of multi_mapping_list in its order, with the candidates
 * target[multi_off[m] .. multi_off[m + 1]) (each < n_targets, duplicates kept, at least one) and weight[m] (the aligned length for meta,
 * 1.0 for trans).  unique[t] is base_count_unique / read_count_unique (an integer below 2^53), total is total_base / total_reads (> 0, an
 * integer below 2^53 / 100), max_iter and factor are 100 and 0.01 (meta) or 1000 and 0.001 (trans); the host enqueues `group` iterations
 * between two looks at the device's stop flag (10 / 50, the reference's print cadence; 0 = 1).  n_multi == 0 is valid.
 * Out: abundance[n_targets] in percent, count[n_targets] (base_count_tmp / read_count_tmp of the last executed iteration),
 * diff_trace[max_iter] (diff_tmp of iteration i; entries from n_iter on are 0), n_iter (iterations executed, 1 .. max_iter), n_nonfinite
 * (abundances of the last iteration that are NaN or infinite: the rest is then meaningless).  TPM and the file are the caller's
 * (nanosim_amd/characterize/quantification.py: em_quantify, format_quantification).  NS_EINVAL for n_targets == 0 and total == 0 (not > 0).
 * Added without an ABI change. */
typedef struct ns_em_problem {
    uint32_t n_targets, n_multi;
    const uint64_t *multi_off;  /* n_multi + 1, from 0 */
    const uint32_t *target;     /* multi_off[n_multi] */
    const double *weight;       /* n_multi */
    const double *unique;       /* n_targets */
    double total, factor;
    uint32_t max_iter, group;
} ns_em_problem;
typedef struct ns_em_result {
    double *abundance;          /* in: host buffer of n_targets entries (out) */
    double *count;              /* in: host buffer of n_targets entries (out) */
    double *diff_trace;         /* in: host buffer of max_iter entries (out) */
    uint32_t n_iter, reserved;  /* out */
    uint64_t n_nonfinite;       /* out */
    double ms_kernel;           /* the whole loop, with the reads of the flag */
} ns_em_result;
int ns_em_quantify(ns_ctx *ctx, const ns_em_problem *p, ns_em_result *out);

/* ---- training side: the intron-retention model, the Markov counts ---------------------------------------------------------------------------------
 * replaces the loop of intron_retention (src/model_intron_retention.py, M:104-176) over every read that has a genome alignment and a
 * transcriptome alignment; nanosim_amd/csrc/ns_ir_train.h says how, with every corner of the reference that is kept.
 * Per read r = 0 .. n_reads - 1: the CIGAR text of its genome alignment, start[r] its 0-based reference start, chrom[r] the id of its
 * chromosome among those that carry introns (< n_chrom) or NS_IR_NONE when none lives on it, trx[r] the id of its transcript (< n_trx)
 * or NS_IR_NONE when the annotation has no intron for it.  Per transcript t (ns_ir_introns): its introns intr_off[t] .. intr_off[t + 1] - 1
 * in the order of the annotation (chromosome id, 0-based start, end) and the union of them as intervals merged_off[t] ..
 * merged_off[t + 1] - 1, sorted by (chromosome, start), none empty, no two overlapping or touching.
 * Out: first[2] (the first intron of a counted read: [0] not retained, [1] retained), states[4] ([2 * previous + current] for every later
 * intron), state[n_reads] (NS_IR_READ_NONE: nothing counted, NS_IR_READ_NO_IR: counted without a retained intron, NS_IR_READ_IR:
 * counted with one or more), retained[ceil(introns / 32)] (bit i & 31 of word i >> 5: intron i — an index into intr_* — is retained by at
 * least one read).  A BAD CIGAR (empty, an unknown op, a count without an op or the reverse, a reference position beyond 2^32 - 1) is
 * counted in n_bad, first_bad the smallest index of one (n_reads without); such a read counts nothing.  n_reads == 0 is valid.
 * NS_EINVAL for offsets that do not ascend from 0 and ids out of range.  Added without an ABI change. */
#define NS_IR_NONE 0xFFFFFFFFu
#define NS_IR_READ_NONE 0
#define NS_IR_READ_NO_IR 1
#define NS_IR_READ_IR 2
typedef struct ns_ir_introns {
    uint32_t n_trx, n_chrom;
    const uint64_t *intr_off;       /* n_trx + 1, from 0 */
    const uint32_t *intr_chrom, *intr_start, *intr_end;          /* intr_off[n_trx] each */
    const uint64_t *merged_off;     /* n_trx + 1, from 0 */
    const uint32_t *merged_chrom, *merged_start, *merged_end;    /* merged_off[n_trx] each */
} ns_ir_introns;
typedef struct ns_ir_train_result {
    uint8_t *state;             /* in: host buffer of n_reads entries (out) */
    uint32_t *retained;         /* in: host buffer of ceil(intr_off[n_trx] / 32) words (out) */
    uint64_t first[2];          /* out */
    uint64_t states[4];         /* out */
    uint64_t n_bad, first_bad;  /* out */
    double ms_kernel;
} ns_ir_train_result;
int ns_ir_train(ns_ctx *ctx, const uint8_t *cigar, const uint64_t *cigar_off, const uint32_t *start, const uint32_t *chrom,
                const uint32_t *trx, uint32_t n_reads, const ns_ir_introns *introns, ns_ir_train_result *out);

/* ---- training side: the best hit per read of LAST's MAF alignments -------------------------------------------------------------------------------
 * replaces besthit_and_unaligned of src/get_besthit_maf.py (G:8-56) up to the lengths of the unaligned reads; nanosim_amd/csrc/ns_maf_best.h
 * says how.  text[nbytes]: a MAF file as it is, or what `grep '^s '` leaves of it.  An `s` line begins at the first byte of the text or
 * behind a '\n' with `s` and a space or a tab; everything else is skipped.  The `s` lines are pairs (reference line, query line); fields
 * are separated like Python's split(); `start`, `size` and `srcSize` are decimal digits that fit 32 bits, a line with anything else there or
 * with fewer than 7 fields is BAD.  Of the pairs of a query name the one with the largest `size` is KEPT, of several the first in the text.
 * names / names_off / n_names (optional; n_names == 0 without): the names of a reads file one behind the other, name i the bytes
 * names_off[i] .. names_off[i + 1] - 1; found[i] = 1 when name i is the query name of a pair, else 0.
 * Out: n_lines, n_pairs, n_kept (= the reference's num_aligned), pos_strand (kept pairs whose two strand fields are equal byte strings), and
 * per kept pair, in the order of the text, lines / records / figures — all offsets are offsets into text.  These three arrays belong to
 * the context and stay valid until the next ns_maf_besthit on it or ns_destroy.
 * An odd n_lines is NS_EINVAL (n_lines is set).  With a bad line the call returns NS_OK, first_bad_line is the index of the first one among the
 * `s` lines and first_bad_offset where it begins (n_lines and ~0 without), and nothing is counted: n_kept == 0, found untouched.
 * NS_EINVAL for 2^31 pairs or more and offsets that do not ascend from 0, NS_ENOMEM when the device cannot hold the text and the
 * tables.  nbytes == 0 is valid and keeps nothing.  ms_kernel: from the first kernel to the last, the waits of the host for the number of
 * lines and for the bad-line check included.  Added without an ABI change. */
typedef struct ns_maf_best_lines {      /* the two lines of a kept pair, each with its '\n' where it has one */
    uint64_t ref_begin, ref_end, qry_begin, qry_end;
} ns_maf_best_lines;
typedef struct ns_maf_best_record {     /* what characterize.maf_records takes from the two lines: name and start of the reference, the two sequences */
    uint64_t ref_name_at, ref_seq_at, qry_seq_at;
    uint32_t ref_name_len, ref_seq_len, qry_seq_len, ref_start;
} ns_maf_best_record;
typedef struct ns_maf_best_figures {    /* src/head_align_tail_dist.py:91-110: r[3], r[5], q[2], q[5], q[5] - q[3] */
    uint32_t aligned_ref, ref_total, head, total;
    int64_t ht;
} ns_maf_best_figures;
typedef struct ns_maf_best_result {
    uint8_t *found;                         /* in: host buffer of n_names bytes (out); may be NULL when n_names == 0 */
    const ns_maf_best_lines *lines;         /* out: n_kept entries each, owned by the context */
    const ns_maf_best_record *records;
    const ns_maf_best_figures *figures;
    uint64_t n_lines, n_pairs, n_kept, pos_strand;          /* out */
    uint64_t first_bad_line, first_bad_offset;              /* out */
    double ms_kernel;
} ns_maf_best_result;
int ns_maf_besthit(ns_ctx *ctx, const uint8_t *text, uint64_t nbytes, const uint8_t *names, const uint64_t *names_off, uint32_t n_names,
                   ns_maf_best_result *out);

/* ---- training side: BAM records to SAM text ----------------------------------------------------------------------------------------------------
 * the records of a BAM file as `samtools view` prints them, byte for byte; nanosim_amd/csrc/ns_bam.h has the record layout, the rules of
 * the text and how the kernels work.  bytes[nbytes]: inflated BAM that begins at a record boundary (the header is the caller's).  The call
 * hops the block_size chain; `consumed` counts the bytes of the whole records.  A trailing partial record is left unconsumed when
 * final == 0 and is a bad record (NS_BAM_BAD_TRUNCATED) when final != 0.  ref_names / ref_off / n_ref: the names of the header's reference
 * dictionary one behind the other, name i the bytes ref_off[i] .. ref_off[i + 1] - 1.
 * Out: text[n_text], the lines of the n_records records, each with its '\n'; line_off[n_records + 1], where they begin in text
 * (line_off[n_records] == n_text).  Both belong to the context, lie in page-locked host memory and stay valid until the next ns_bam_to_sam
 * on it or ns_destroy.  With a bad record the call returns NS_OK and emits nothing (n_records == n_text == consumed == 0): first_bad is its
 * index among the records of this call (~0 without), first_bad_offset where its block_size stands in bytes, bad_reason why.
 * NS_EINVAL for null arguments, offsets that do not ascend from 0 and 2^31 records or more, NS_ENOMEM when the device cannot hold the
 * batch.  nbytes == 0 is valid.  ms_kernel: from the first kernel to the last, the waits of the host for the bad-record check, for the
 * text of the floats and for the size of the text included.  Added without an ABI change. */
enum { NS_BAM_OK = 0, NS_BAM_BAD_BLOCK_SIZE = 1, /* block_size is negative or smaller than what the record's own counts need */
       NS_BAM_BAD_LSEQ = 2,                      /* l_seq < 0 */
       NS_BAM_BAD_REFID = 3,                     /* refID or next_refID outside [-1, n_ref) */
       NS_BAM_BAD_NAME = 4,                      /* the name is not NUL-terminated */
       NS_BAM_BAD_TAG_TYPE = 5,                  /* a tag, or the elements of a B tag, of an unknown type */
       NS_BAM_BAD_TAG_NUL = 6,                   /* a Z or H tag without a NUL inside the record */
       NS_BAM_BAD_TAG_COUNT = 7,                 /* a B tag's count, or a tag's value, runs past the record */
       NS_BAM_BAD_TRUNCATED = 8 };               /* final != 0 and the bytes end inside a record */
typedef struct ns_bam_result {
    const uint8_t *text;                         /* out, owned by the context */
    const uint64_t *line_off;
    uint64_t n_records, n_text, consumed;        /* out */
    uint64_t first_bad, first_bad_offset;        /* out */
    uint32_t bad_reason, reserved;
    double ms_kernel;
} ns_bam_result;
int ns_bam_to_sam(ns_ctx *ctx, const uint8_t *bytes, uint64_t nbytes, int final, const uint8_t *ref_names, const uint64_t *ref_off, uint32_t n_ref,
                  ns_bam_result *out);

/* ---- training side: cs and MD tags from the reference genome -----------------------------------------------------------------------------------
 * the MD:Z text (samtools calmd's algorithm) and the short-form cs:Z text (minimap2 --cs) of n alignments from CIGAR, POS, SEQ and the
 * reference set with ns_set_reference / ns_set_reference_device (the engine's normalised copy of it); nanosim_amd/csrc/ns_calmd.h has the
 * rules of the text and how the kernels work.  Record i: the CIGAR text cigar[cigar_off[i] .. cigar_off[i + 1]), SEQ likewise, chrom[i] the
 * index of its chromosome in the set reference, pos[i] its 1-based POS.
 * Out: md[md_off[n]] and cs[cs_off[n]], the texts one behind the other without separators, text i at md_off[i] .. md_off[i + 1] - 1; all
 * four belong to the context, lie in page-locked host memory and stay valid until the next ns_calmd on it or ns_destroy.  A bad record has
 * empty texts; the call returns NS_OK and reports their number (n_bad), the index of the first (first_bad; ~0 without) and why that one is
 * bad (bad_reason).  NS_EINVAL: no reference set, a null argument, offsets that do not ascend from 0, 2^31 records or more.  n == 0 is
 * valid (md_off[0] == cs_off[0] == 0).  ms_kernel: from the first kernel to the last, the wait of the host for the sizes of the texts
 * included.  Added without an ABI change. */
enum { NS_CALMD_OK = 0, NS_CALMD_BAD_CIGAR = 1,  /* the CIGAR does not parse (a count of 0 or of 2^28 or more included) */
       NS_CALMD_BAD_OP = 2,                      /* an op outside MIDSH=X */
       NS_CALMD_BAD_CLIP = 3,                    /* an S that is not outermost inside the H ops (or an H inside) */
       NS_CALMD_BAD_SEQ_LEN = 4,                 /* the length of SEQ is not the sum of its S/M/=/X/I ops */
       NS_CALMD_BAD_SEQ_BYTE = 5,                /* a SEQ byte that is not a letter */
       NS_CALMD_BAD_CHROM = 6,                   /* chrom outside the set reference */
       NS_CALMD_BAD_POS = 7,                     /* POS 0 */
       NS_CALMD_BAD_END = 8,                     /* the alignment runs past the end of its chromosome */
       NS_CALMD_BAD_NO_COLUMN = 9 };             /* no M / = / X column at all */
typedef struct ns_calmd_result {
    const uint8_t *md;                           /* out, owned by the context */
    const uint64_t *md_off;
    const uint8_t *cs;
    const uint64_t *cs_off;
    uint64_t n_bad, first_bad;
    uint32_t bad_reason, reserved;
    double ms_kernel;
} ns_calmd_result;
int ns_calmd(ns_ctx *ctx, const uint8_t *cigar, const uint64_t *cigar_off, const uint8_t *seq, const uint64_t *seq_off,
             const uint32_t *chrom, const uint32_t *pos, uint32_t n, ns_calmd_result *out);

/* ---- training side: the index of a SAM text ------------------------------------------------------------------------------------------------------
 * where the lines, the fields and the tags cs:Z: MD:Z: NM:i: SA:Z: of a SAM text stand in its bytes, so that no reader splits a line;
 * nanosim_amd/csrc/ns_sam_index.h has the rules (those of characterize.sam_text) and how the kernels work.  text[nbytes]: SAM text that
 * begins at a line start.  A line begins at byte 0 or behind a '\n'; one whose first byte is `@` is a header line, wherever it stands;
 * every other line, an empty one included, is a record.  Fields are what split("\t") gives.  Of the fields 11 onwards that begin with one
 * of the four prefixes the last one is the tag.  FLAG, POS and the NM value are parsed when they are 1-10 decimal digits below 2^32;
 * anything else only sets the row's NS_SAM_*_ODD bit, and the caller decides what the text means.
 * Out: rows[n_records], one per record in the order of the text, and header[n_header], the header lines; both belong to the context and
 * stay valid until the next ns_sam_index on it or ns_destroy.  n_odd: the bytes of the text that are '\r' or >= 0x80 (text mode is not
 * restated: the caller turns such a text away).  n_cs / n_md: the records that carry the tag.
 * NS_EINVAL for null arguments, a line of 2^32 bytes or more and 2^32 lines or more, NS_ENOMEM when the device cannot hold the text and
 * the lists.  nbytes == 0 is valid and has no rows.  ms_kernel: from the first kernel to the last, the wait of the host for the number of
 * lines and tabs included.  Added without an ABI change. */
enum { NS_SAM_FLAG_ODD = 1, NS_SAM_POS_ODD = 2, NS_SAM_NM_ODD = 4,          /* ns_sam_row.bits: the number is not plain (flag / pos / nm are 0) */
       NS_SAM_HAS_CS = 16, NS_SAM_HAS_MD = 32, NS_SAM_HAS_NM = 64, NS_SAM_HAS_SA = 128 };   /* ... the record has the tag */
typedef struct ns_sam_row {             /* everything but begin and end is relative to begin */
    uint64_t begin, end;                /* the line in text; end: its '\n' or nbytes */
    uint32_t n_fields, bits;
    uint32_t field_end[11];             /* where fields 0 .. 10 end; field k + 1 begins one behind; end - begin for a field the line has not */
    uint32_t flag, pos, nm;
    uint32_t tag_at[4], tag_len[4];     /* the values of cs, MD, NM, SA, behind their five prefix bytes (0, 0 without the tag) */
} ns_sam_row;
typedef struct ns_sam_span { uint64_t begin, end; } ns_sam_span;          /* a header line, without its '\n' */
typedef struct ns_sam_index_result {
    const ns_sam_row *rows;             /* out, owned by the context */
    const ns_sam_span *header;
    uint64_t n_records, n_header, n_odd, n_cs, n_md;                       /* out */
    double ms_kernel;
} ns_sam_index_result;
int ns_sam_index(ns_ctx *ctx, const uint8_t *text, uint64_t nbytes, ns_sam_index_result *out);

/* ---- compressed output: BGZF members, deflated on the GPU before the copy (nanosim_amd/csrc/ns_gz.h) ----
 * A BGZF file is a series of independent gzip members of at most 64 KiB each; any concatenation of members is a valid .gz file.  Here
 * every member holds at most NS_GZ_BLOCK_BYTES input bytes as ONE deflate block: a dynamic-Huffman block of literals only (no matches),
 * or a stored block when that is smaller or when the code lacks a byte of the block.  One code serves a whole stream of blocks.
 *
 * ns_gz_code: a length-limited (<= 15 bits) canonical Huffman code over the byte values whose count is not 0, plus end-of-block
 * (index 256).  len[v] == 0: the value has no code.  code[v]: the code bit-reversed, as deflate packs it (first bit of the code in bit
 * 0).  header[]: the complete header of the dynamic block as a bit string of header_bits bits, first bit in bit 0 of header[0], zero
 * behind the last bit: BFINAL = 1, BTYPE = 2, HLIT = 0 (257 codes), HDIST = 0 (one distance code of length 0: all literals), HCLEN, the
 * lengths of the code-length code and the 258 run-length-coded lengths.  Its worst case is 3 + 5 + 5 + 4 bits, 19 x 3 bits, and at most
 * 7 bits for every one of the 258 lengths (a repeat symbol with its extra bits, 14 bits at most, stands for three lengths or more):
 * 17 + 57 + 1806 = 1880 bits = 235 bytes, kept in NS_GZ_HEADER_BYTES = 240 (whole 32-bit words).
 * ns_gz_code_build needs no context and no GPU.  NS_EINVAL for a null argument. */
#define NS_GZ_BLOCK_BYTES 16384u
#define NS_GZ_HEADER_BYTES 240u
typedef struct ns_gz_code {
    uint8_t len[257];
    uint16_t code[257];
    uint32_t header_bits;
    uint8_t header[NS_GZ_HEADER_BYTES];
} ns_gz_code;
int ns_gz_code_build(const uint64_t hist[256], ns_gz_code *out);
/* an upper bound of what nbytes input bytes in n_ranges ranges compress to (every block stored, one short block more per range) */
uint64_t ns_gz_bound(uint64_t nbytes, uint32_t n_ranges);
/* the counts of the 256 byte values in the record image (which = NS_BUF_RECORDS) or the error-profile image (NS_BUF_ERRLOG) of the last batch */
int ns_gz_histogram(ns_ctx *ctx, int which, uint64_t hist[256]);
/* cuts[n_cuts]: ascending byte offsets into src[nbytes].  Every range [cuts[i], cuts[i + 1]) becomes a whole number of members, one
 * behind the other in dst; gz_off[i], i < n_cuts - 1, is where the members of range i begin, gz_off[n_cuts - 1] where the last ones
 * end.  An empty range has no bytes.  code == NULL: the code is built from the counts of src.  Host bytes in, host bytes out, on the
 * kernels of ns_gz_result.  NS_EINVAL for null arguments, n_cuts == 0, cuts that do not ascend or lie beyond nbytes, and when dst_cap is
 * smaller than the result (gz_off is filled then: gz_off[n_cuts - 1] is the size needed). */
int ns_gz_bytes(ns_ctx *ctx, const uint8_t *src, uint64_t nbytes, const uint64_t *cuts, uint32_t n_cuts, const ns_gz_code *code,
                uint8_t *dst, uint64_t dst_cap, uint64_t *gz_off);
/* ... the same of the record image (which = NS_BUF_RECORDS) or the error-profile image (NS_BUF_ERRLOG) of the LAST batch, into the result
 * buffer NS_BUF_RECORDS_GZ / NS_BUF_ERRLOG_GZ of the batch's result slot: ns_copy_out, ns_sink_write_range and ns_device_ptr take the two
 * ids like the plain images, and the slot rule of the plain images holds for them.  NS_ESTATE without a batch. */
enum { NS_BUF_RECORDS_GZ = 7, NS_BUF_ERRLOG_GZ = 8 };
int ns_gz_result(ns_ctx *ctx, int which, const uint64_t *cuts, uint32_t n_cuts, const ns_gz_code *code, uint64_t *gz_off);

/* device address of a result buffer (for zero-copy consumers such as torch / RCCL); NULL if absent */
const void *ns_device_ptr(ns_ctx *ctx, int which);

#ifdef __cplusplus
}
#endif
#endif /* NANOSIM_AMD_H */
