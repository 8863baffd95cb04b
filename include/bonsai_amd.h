/*
 * bonsai_amd.h -- C ABI of the MI355X-native Bonsai classify hot path.
 *
 * Drop-in boundary.  The reference (dnbaker/bonsai) has no FFI layer: the path sits
 * behind C++ templates.  Each entry point below names the reference interface it replaces
 * (file:line into the reference checkout).  Plain pointers and sizes only, int error codes, no
 * exceptions cross this boundary, one context per device, calls on one context are serialised by the
 * caller.  All multi-byte data is little-endian host order.
 *
 * Host-pointer entry points copy in/out and synchronise before returning.  The `_device` entry points
 * take HIP device pointers plus a hipStream_t (passed as void*) and only enqueue work.
 */
#ifndef BONSAI_AMD_H
#define BONSAI_AMD_H
#include <stdint.h>
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct bns_ctx bns_ctx;

enum {
    BNS_OK = 0,
    BNS_ERR_ARG = -1,            /* bad argument (k out of [1,32], NULL pointer, ...) */
    BNS_ERR_HIP = -2,            /* HIP runtime failure; see bns_last_error() */
    BNS_ERR_NOMEM = -3,          /* device or host allocation failed */
    BNS_ERR_STATE = -4,          /* table / taxonomy / spacer not loaded yet */
    BNS_ERR_TAX_CYCLE = -5,      /* parent[] contains a cycle (the reference would loop forever) */
    BNS_ERR_TAX_RANGE = -6,      /* taxid >= 2^28: flat parent[] cap */
    BNS_ERR_TABLE = -7,          /* khash arrays inconsistent (n_buckets not a power of two, unreachable key) */
    BNS_ERR_NO_DEVICE = -8       /* no usable gfx950 device */
};

/* table layouts in HBM (bns_load_table*) */
enum {
    BNS_LAYOUT_KHASH  = 0,  /* probe the on-disk SoA arrays as they are: Wang64 + triangular probing, khash64.h:250-263 */
    BNS_LAYOUT_BUCKET = 1,  /* re-hash on device into 64-byte buckets of 4 x {key,val,occ}; same key->value map */
    BNS_LAYOUT_MINBUCKET = 2 /* (default) 128-byte buckets {u64 keys[10], u32 vals[10], u32 count|occupancy, u32 S}.  The home
                                bucket of a key comes from its minimizer -- the smallest hash among the canonical m-mers inside
                                the k-mer, m = k-15, k-11 or k-8 as the db allows (never below 16 / 19 / 19: m = k for small k;
                                spaced seeds: m-mers of the mask's longest run; see bns_set_minimizer_span) -- so neighbouring k-mers
                                of a read share a 128-byte line; inside a bucket the key sits at the slot a per-bucket
                                perfect-hash multiplier S assigns it; a full bucket spills to the next one (at most 4), then to
                                a small plain-hashed overflow table.  Same key->value map.  Needs bns_set_encoder() before the
                                table is loaded (the layout depends on k). */
};

#define BNS_TAX_ABSENT 0xFFFFFFFFu   /* parent[] entry of an id that is not a key of the parent map */

/* ---- lifecycle ------------------------------------------------------------------------------ */
/* Replaces: ClassifierGeneric ctor (classifier.h:155-166) + ForPool (util.h:109-118): the context owns
 * the device, its stream and all device allocations. */
int  bns_create(int device, bns_ctx **out);
int  bns_device_count(void);            /* visible HIP devices (0 when there is none) */
/* PCI address of a device ("0000:05:00.0", what /sys/bus/pci/devices/ lists it under): lets a host bind its threads to the CPUs
 * next to the GPU (.../local_cpulist) before it creates a context.  cap >= 16. */
int  bns_device_pci_bus_id(int device, char *out, int cap);
void bns_destroy(bns_ctx *ctx);
const char *bns_strerror(int code);
const char *bns_last_error(const bns_ctx *ctx);     /* detail of the last failure on this context */
int  bns_version(void);

/* ---- encoder configuration -------------------------------------------------------------------- */
/* Replaces: Spacer(k, w=k, spaces) (spacer.h:58-71) + Encoder(const Spacer&, bool canonicalize)
 * (encoder.h:153) as classify builds them (bin/bonsai.cpp:152-153).  gaps = k-1 "extra gap" values as
 * stored in bns.db (database.h:46-48), NULL = contiguous.  A spaced seed is never canonicalised
 * (encoder.h:148-150).  spaced_intended: 0 reproduces the reference's string for_each (a spaced seed
 * emits nothing); 1 = for_each_uncanon_spaced semantics (encoder.h:233-239). */
int bns_set_encoder(bns_ctx *ctx, uint32_t k, const uint16_t *gaps, int canonicalize, int spaced_intended);

/* Replaces: the window argument of Spacer(k, w, spaces) (spacer.h:58-71) and the Encoder's ScoreType template
 * argument (encoder.h:113): windowed minimizer selection as `bonsai build -w <w> [-e]` uses it
 * (bin/bonsai.cpp:226-261 -> feature_min.h:67-82 -> Encoder::for_each_canon_windowed, encoder.h:211-217; with
 * canonicalize = 0 for_each_uncanon_unspaced_windowed, encoder.h:273-306, whose windows run over the emitted k-mers;
 * a spaced seed goes through for_each_uncanon_spaced, encoder.h:233-239).
 * Honoured by bns_encode_batch* and bns_build_table_device; classify always looks up every k-mer (w = k,
 * bin/bonsai.cpp:152).  w <= comb size = unwindowed.  At most 1024 k-mers per window.
 *   BNS_SCORE_LEX           score::Lex = FRev64 (encoder.h:47) -- restated from the un-vendored sketch library,
 *                           parity unpinned
 *   BNS_SCORE_ENTROPY_PATH  score::Entropy as the path overloads compute it: (u64)(i64)(double(kmer)/(-1+1e-4))
 *                           
 *   BNS_SCORE_ENTROPY_STRING score::Entropy as the STRING overload computes it for a contiguous seed
 *                           (for_each_[un]canon_unspaced_windowed_entropy_, encoder.h:307-353): (u64)(double(fwd_kmer) /
 *                           (sum over the k-mer's bases of (n/k) ln(n/k) + .001)); like the -C windowed stream its windows
 *                           run over the emitted k-mers, selection is on forward k-mers and the emitted value is
 *                           canonicalised when canonicalize = 1.  Parity unpinned to the last ulp of the sum (the
 *                           reference adds in hash-map order; here A, C, G, T) */
enum { BNS_SCORE_LEX = 0, BNS_SCORE_ENTROPY_PATH = 1, BNS_SCORE_ENTROPY_STRING = 2 };
int bns_set_window(bns_ctx *ctx, uint32_t w, int score);

/* ---- database --------------------------------------------------------------------------------- */
/* Replaces: Database<khash_t(c)>(path).db_ (database.h:33-56 -> util.h:334-364 khash_load_impl): the
 * three khash arrays exactly as they sit in bns.db.  flags has max(1, n_buckets>>4) words.  For the re-hashed layouts the arrays
 * are uploaded whole when they fit the HBM next to the table they are turned into, and streamed from these host buffers in
 * chunks of 2^27 slots when they do not (an 8e9-key db: 210 GB of arrays, 200+ GB of table); BNS_LAYOUT_KHASH keeps them resident. */
int bns_load_table(bns_ctx *ctx, uint64_t n_buckets, const uint32_t *flags, const uint64_t *keys,
                   const uint32_t *vals, int layout);
/* ---- the `void *stream` argument of the _device entry points, bns_build_add, bns_build_minimize_add, bns_build_count_add and bns_windows_add
 * `stream` is a hipStream_t of the context's device; NULL means the context's own stream (the one every host-buffer entry point
 * works on).  For a non-NULL stream:
 *   ORDER     everything the call enqueues -- kernels, memsets, the copies of its counters -- goes on `stream`, in order.  Inputs
 *             written by work enqueued on `stream` before the call are seen (the caller need not wait for them); the results are
 *             complete for work enqueued on `stream` after the call returns.  Nothing is ordered against any other stream.
 *   RETURN    these return with their work still queued: bns_probe_device, bns_encode_batch_device, bns_windows_add (unless the
 *             session began with timing on: a timed add waits for its batch), and bns_classify_batch_device /
 *             bns_classify_batch_packed_device when max_read_len is given AND no unit can hold more than 128 k-mers
 *             (mates * (max_read_len - seed span + 1) <= 128: no overflow list to read back).  Their inputs and outputs are the
 *             device's until `stream` has been waited for.  These have synchronised `stream` when they return:
 *             bns_load_table_device, bns_build_table_device, bns_build_add, bns_build_minimize_add, bns_build_count_add, and the two classify calls
 *             with max_read_len = 0 (the longest read is read back) or with units of more than 128 k-mers (the overflow count is).
 *             bns_build_add, bns_build_minimize_add, bns_build_count_add and bns_windows_add first wait for the context's own stream (begin, seed, a
 *             reset or an earlier grow worked there).
 *   WORKSPACE a context has ONE workspace (its counters, records, packed image, flag words, scratch, overflow list, tally and
 *             sketches), shared by all its calls.  Two calls on one context on different streams must not overlap: ordering them
 *             (an event, or waiting for the first) is the caller's job.  A call that has to enlarge a workspace buffer frees the old
 *             one, which drains the device.
 *   READERS   bns_tally_read, bns_sketch_read, bns_build_finish / bns_build_export and bns_dev_download work on the context's own
 *             stream: `stream` must be complete before they are called.  bns_windows_read and bns_dev_sync drain the device
 *             themselves.  The timing events (bns_set_timing) are recorded on `stream`, around the call's dominant kernel. */

/* Same, arrays already resident in HBM (e.g. after an RCCL broadcast).  With BNS_LAYOUT_KHASH the
 * context BORROWS the arrays (caller keeps them alive); with BNS_LAYOUT_BUCKET they are only read
 * during the call's enqueued kernels. */
int bns_load_table_device(bns_ctx *ctx, uint64_t n_buckets, const uint32_t *d_flags, const uint64_t *d_keys,
                          const uint32_t *d_vals, int layout, void *stream);
/* Size of the re-hashed table.  Default (nothing set), BNS_LAYOUT_MINBUCKET: sized from the number of PRESENT keys -- one
 * 128-byte bucket per 0.83 keys (buckets of 10 filled to 1/12: the knee of the load sweep) or what fits in three
 * quarters of the free HBM, whichever is smaller; any bucket count will do (the bucket index is a multiply-high, not a mask), so
 * a RefSeq-scale db takes exactly the memory there is.  BNS_LAYOUT_BUCKET: 2x the khash bucket count in 16-byte slots.
 *   bns_set_bucket_slots_log2  the exact log2 of the size in 16-byte slots (MINBUCKET: 2^(log2-3) buckets), 0 = automatic
 *   bns_set_table_buckets      MINBUCKET: the exact number of buckets a key can call home (>= keys / 9.7), 0 = automatic
 * No reference counterpart: the key -> value map is the same whatever the size. */
int bns_set_bucket_slots_log2(bns_ctx *ctx, uint32_t log2_slots);
int bns_set_table_buckets(bns_ctx *ctx, uint64_t n_home_buckets);
/* Multi-GPU load (the seam is process_dataset, classifier.h:296-337): the same table in n_ctx contexts, one per
 * device.  The khash arrays cross PCIe ONCE (into ctxs[0]'s device) and reach the other devices by an RCCL broadcast over xGMI
 * (librccl is opened on first use, only when two different devices take part); every device then builds its own clustered
 * layout, all of them at the size and with the minimizer window ctxs[0] chose.  Contexts that share a device (a one-GPU box exercising this path) are fed
 * by device-to-device copies instead -- RCCL admits a device once per communicator.  n_ctx == 1 is bns_load_table.  On failure no
 * context keeps a table and bns_last_error(ctxs[0]) holds the failing context's message.  A db whose
 * arrays do not fit the HBM next to its table is not replicated array by array: every context streams the host buffers into its own
 * table (as bns_load_table does), the first alone -- its table size is everyone's -- the others side by side. */
int bns_load_table_multi(bns_ctx **ctxs, int n_ctx, uint64_t n_buckets, const uint32_t *flags, const uint64_t *keys,
                         const uint32_t *vals, int layout);

/* What the last bns_load_table_multi broadcast ran on: librccl's version code (ncclGetVersion: e.g. 22606; 0 before the library was
 * opened) and the number of ranks of its communicator (0: no broadcast yet -- one context, or a db streamed per device).  A host prints
 * it so that a multi-GPU record says which collective library replicated the table over how many devices. */
int bns_rccl_info(int *version, int *n_ranks);
/* number of present keys / device bytes of the active table.  n_keys is counted when the table is loaded, in every layout (a
 * BNS_LAYOUT_KHASH load passes over the flag words once for it); bns_table_tally's sum(direct) equals it. */
int bns_table_info(const bns_ctx *ctx, uint64_t *n_keys, uint64_t *device_bytes, int *layout);
/* stats4 = {present keys, keys in the MINBUCKET overflow table, main table bytes, overflow table bytes} */
int bns_table_stats(const bns_ctx *ctx, uint64_t *stats4);

/* The MINBUCKET table's minimizer window for contiguous seeds, span = k - m.  0 (default): chosen when the table is loaded --
 * the widest of 15, 11, 8 with which fewer than 1 key in 100 misses its home bucket (a db of window minimizers, bonsai build
 * -w 50, takes 15: fewer bucket fetches per read; a db of every k-mer needs 8).  8 / 11 / 15 fix it.  No reference counterpart:
 * the key -> value map is the same whatever the window (tests/test_gpu_ref_golden.py runs all three).  Call before
 * bns_load_table*.  bns_table_minimizer reports m and the number of keys that are not in their home bucket. */
int bns_set_minimizer_span(bns_ctx *ctx, uint32_t span);
int bns_table_minimizer(const bns_ctx *ctx, uint32_t *m, uint64_t *spilled_keys);
/* Width of the minimizer identity the MINBUCKET table orders its m-mers by and derives the bucket from (contiguous seeds):
 * 32 = a 32-bit hash (cheapest per lookup; beyond a few 1e8 minimizer groups distinct groups share hash values, hence buckets,
 * whatever the table size), 52 = hash and m-mer carried through the window minimum as one double (no sharing; what dbs of
 * RefSeq scale need), 0 (default) = chosen when the table is loaded: both forms are tried on a sample of the buckets, and 52 is
 * taken when the 32-bit form leaves more than 2 keys in 100 outside their home bucket and 52 bits at most 60 % of that.  Call
 * before bns_load_table*.  Same key -> value map either way. */
int bns_set_minimizer_identity(bns_ctx *ctx, int bits);
/* How the clustered table is filled: 0 (default) = chosen when the table is loaded, 1 = keys in arrival order, 2 = group by group
 * (whole minimizer groups keep their home bucket, largest first; the header's tag bits say which groups have keys elsewhere:
 * docs/TABLE_LAYOUT.md) -- what the loader takes by itself for a crowded table (more than 1 key in 100 outside its home bucket
 * in its trial pass).  Same key -> value map either way; replicas of a multi-GPU load take the root's choice.  Call before
 * bns_load_table*.  No reference counterpart (khash has one layout: khash64.h:198-263). */
int bns_set_table_fill(bns_ctx *ctx, int mode);
/* geo8 = {buckets a key can call home (MINBUCKET) / buckets (BUCKET, KHASH), minimizer length m, identity bits (32 / 52),
 * keys that are not in their home bucket, the window the table was built with as bns_set_minimizer_span names it (15 / 11 / 8;
 * 0 for a spaced seed), keys in the overflow table, 1 when the table was filled group by group (crowded tables: whole minimizer
 * groups keep their home bucket, largest first), 0}; zeros where the layout has no such thing.  Feeding entries 0, 4, 2 and
 * 6 + 1 to bns_set_table_buckets / bns_set_minimizer_span / bns_set_minimizer_identity / bns_set_table_fill reproduces the table
 * elsewhere. */
int bns_table_geometry(const bns_ctx *ctx, uint64_t *geo8);
/* "" or what the last bns_load_table* had to say about the table it built (e.g. a forced minimizer window whose groups
 * outgrow their buckets: correct results, slower lookups).  Valid until the next load on this context. */
const char *bns_table_warning(const bns_ctx *ctx);

/* Replaces: build_parent_map(nodes.dmp) (util.h:766-785) as a flat array: parent[id] for id in [0,n),
 * BNS_TAX_ABSENT where id is not a key.  parent[1] must already be 0 (util.h:780-781). */
int bns_load_taxonomy(bns_ctx *ctx, const uint32_t *parent, uint32_t n);

/* ---- per-taxon tally (what `bonsai classify -R` reports) ------------------------------------------------------------------------
 * No reference counterpart: the reference counts classified / unclassified reads (classifier.h:138,238) and prints neither.
 * bns_tally_enable(ctx, 1): needs a loaded taxonomy; allocates and zeroes u64 direct[n + 1] (n as given to bns_load_taxonomy).  From then
 * on every classifying entry point (bns_classify_batch, _runs, _device, the _packed three, bns_classify_text and bns_text_finish) adds
 * the units it reports, once each, on the stream of the classify launch: bin 0 = taxon 0 (unclassified); bin t = a taxon t < n whose
 * chain reaches a root with parent 0; bin n = anything else (t >= n, 0xFFFFFFFF, a taxid that is not a key, a broken chain).  Records a
 * call does not take are not counted.  bns_resolve_batch, bns_probe* and the build are not counted.  Reloading the taxonomy zeroes the tally;
 * bns_tally_enable(ctx, 0) frees it.  Off (the default): nothing is launched or allocated.
 * bns_tally_read: len must be n + 1.  direct (may be NULL) receives the counts; clade (may be NULL) the sums over each node's subtree
 * (clade_kernel over the Euler intervals), bins 0 and n as they are.  reset: zero the counts after reading.  Runs on the context's stream;
 * _device calls made on another stream must be complete.  Counts of several contexts add up (clade sums too). */
int bns_tally_enable(bns_ctx *ctx, int on);
int bns_tally_read(bns_ctx *ctx, uint64_t *direct, uint64_t *clade, uint32_t len, int reset);

/* ---- per-taxon key counts of the loaded table (what `bonsai inspect` and `bonsai classify -R -u -d` report) ------------------------
 * No reference counterpart (Kraken 2's kraken2-inspect, the denominator of KrakenUniq's cov column); defined in DESIGN.md.
 * Every key present in the context's active table is counted exactly once, whatever the layout and wherever the loader put it (khash
 * slots that are empty or deleted do not count; home, spill-only and overflow buckets of the clustered layout all do).  A key's value
 * t goes to bns_tally_enable's bins: bin 0 for t = 0; bin t for a taxon t < n whose chain reaches a root; bin n for anything else.
 * The same attribution as bns_sketch_enable's, so a clade's distinct-k-mer estimate over its key count is the share of its keys a
 * sample covered.  direct[v] (may be NULL) = keys in bin v; clade[v] (may be NULL) = the sum over v's subtree (clade_kernel), bins 0 and n
 * as they are.  sum(direct) == bns_table_info's n_keys, always.
 * len must be n + 1, else BNS_ERR_ARG.  No table or no taxonomy: BNS_ERR_STATE.  One streaming walk of the table (inspect_*_kernel) on
 * the context's stream; the scratch is allocated for the call and freed; no state is kept, the tally of bns_tally_enable and the
 * sketches are not touched; nothing is launched or allocated unless this is called.
 * Every context of a multi-GPU load holds the same table: each context's result is the whole answer.  Do NOT add the results of several
 * contexts up (unlike bns_tally_read's). */
int bns_table_tally(bns_ctx *ctx, uint64_t *direct, uint64_t *clade, uint32_t len);

/* ---- confidence threshold (what `bonsai classify -t` sets) -------------------------------------------------------------------------
 * No reference counterpart: Kraken 2's --confidence, as defined in DESIGN.md.  theta = num / den, exact.  For each unit, Q = its hits +
 * its missing k-mers (every k-mer made only of A/C/G/T; ambig does not enter), R = ceil(theta * Q) in integers; the resolved taxon T
 * becomes the first of T, parent(T), ... whose clade (hits equal to it or inside its subtree, u32 counts) holds >= R hits, and 0 when
 * the walk passes a root first.  T stays when R = 0, T = 0, or T is not a node whose chain reaches a root (bns_tally_enable's bin n).
 * Only the taxon changes: missing, ambig, n_hits and the hits stay.  Every classifying entry point (those bns_tally_enable lists)
 * applies it on the stream of the classify launch (confidence_kernel, before the results are unpacked), so the tally counts the new
 * taxa; a call that takes no hits has them written to a buffer of the context's (4 bytes per base).
 * den > 0 and num <= den, else BNS_ERR_ARG.  num > 0 needs a loaded taxonomy, else BNS_ERR_STATE.  num = 0 turns it off (the default):
 * nothing is launched or allocated.  Reloading the taxonomy keeps the setting.  bns_resolve_batch and bns_probe* are not affected. */
int bns_set_confidence(bns_ctx *ctx, uint64_t num, uint64_t den);

/* ---- minimum hit groups (what `bonsai classify -M` sets; version 115) ---------------------------------------------------------------
 * No reference counterpart, and no parity with Kraken 2's --minimum-hit-groups (runs of one minimizer) is claimed: this project's own
 * definition, DESIGN.md.  For each unit, G = the number of DISTINCT keys among the k-mers of all its mates that classify looks up and
 * finds in the table.  The key is what is looked up: the canonical k-mer, the forward k-mer when the encoder is not canonical, the
 * spaced key of a spaced seed, nothing for a spaced seed without spaced_intended; over the image classify saw (after a minimum base
 * quality and bns_set_dust).  A key found at several positions, or in both mates, counts once; no order enters.  After the vote, its
 * overflow pass and the confidence walk, the taxon of a unit becomes 0 when it was not 0 and G < n.  Only the taxon changes: missing,
 * ambig, n_hits and the hits stay.  Needs no taxonomy of its own: a taxon that is no node (0xFFFFFFFF included) is zeroed like any other.
 * Every classifying entry point (those bns_tally_enable lists) applies it on the stream of the classify launch (hit_groups_kernel,
 * behind confidence_kernel and before the results are unpacked), so the tally counts the new taxa; the sketches go by each k-mer's own
 * value and do not change.  ASCII input is packed first (pack_kernel into the context's workspace; once when the sketches are on too);
 * the hit stream is not needed.
 * n in [0, 64], else BNS_ERR_ARG.  n = 0 (the default) and n = 1 (a taxon implies a hit) launch, allocate and read nothing.  While a
 * build or window session is open: BNS_ERR_STATE; bns_windows_begin* return BNS_ERR_STATE while n > 0 (a window's distinct-key count
 * cannot be read from the session's prefix ranges).  Per context; table and taxonomy reloads keep it.  bns_resolve_batch and bns_probe*
 * are not affected. */
int bns_set_min_hit_groups(bns_ctx *ctx, uint32_t n);

/* ---- distinct k-mers per taxon (what `bonsai classify -R -u` reports) --------------------------------------------------------------
 * No reference counterpart (Kraken 2's --report-minimizer-data, KrakenUniq); defined in DESIGN.md.  One HyperLogLog sketch per bin.
 * What is counted: every unit a classify launch processes (the entry points bns_tally_enable lists), every k-mer classify looks up:
 * each k-window of a read made only of unmasked A/C/G/T -- window = k whatever bns_set_window says, the canonical form when the
 * encoder is canonical, the spaced key when it is spaced, nothing for a spaced seed without spaced_intended, both mates of a pair.
 * A key found with value t goes to the sketch of bin t for a taxon t < n whose chain reaches a root, bin 0 for t = 0, bin n otherwise
 * (bns_tally_enable's bins): by the k-mer's own value, not the read's call, so bns_set_confidence does not change it; a minimum
 * base quality does (the masked image).  Units classified twice (a text call that rolls a batch back) change nothing.
 * Sketch: m = 4096 registers of one byte.  For key x (uint64_t): h = fmix64(x), MurmurHash3's finaliser (x ^= x >> 33;
 * x *= 0xff51afd7ed558ccd; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53; x ^= x >> 33); register j = h >> 52; w = h << 12; rho = 53 when w == 0,
 * else clz(w) + 1; reg[j] = max(reg[j], rho).  No arrival order enters: the bytes are exactly reproducible.
 * Estimate (host, double): alpha = 0.7213 / (1 + 1.079 / m); E = alpha m^2 / sum(2^-reg[j]); when E <= 2.5 m and V > 0 registers are 0,
 * E = m ln(m / V); the result is floor(E + 0.5); 0 for an all-zero sketch.  A clade's (or several contexts') sketch is the
 * register-wise maximum of its bins'; bins 0 and n have no subtree.
 * bns_sketch_enable(ctx, max_taxa): needs a loaded taxonomy, else BNS_ERR_STATE; allocates max_taxa sketches of 4 KiB, uint32_t
 * slot_of[n + 1] and seen[n + 1], all zero.  Behind every classify launch, on its stream: the bins of the launch's hits are marked,
 * those seen for the first time take the next free sketches in ascending bin order, then the k-mers are looked up again and added.
 * When the sketches run out the remaining bins get none and their k-mers are not sketched (n_dropped_bins counts them): which bins
 * those are is decided by the sequence of launches alone.  A call that takes no hits has them written to a buffer of the context's
 * (4 bytes per base, shared with bns_set_confidence).  max_taxa = 0 frees everything and turns it off (the default): nothing is
 * launched, allocated or read.  Reloading the taxonomy zeroes the sketches.
 * bns_sketch_read: bins[cap] receives the sketched bins in ascending order, registers[4096 * cap] their sketches in the same order;
 * either may be NULL (both: only the counts).  cap < *n_sketched: BNS_ERR_ARG, with *n_sketched set.  reset: registers, seen and slots
 * back to zero after reading.  Runs on the context's stream, like bns_tally_read. */
int bns_sketch_enable(bns_ctx *ctx, uint32_t max_taxa);
int bns_sketch_read(bns_ctx *ctx, uint32_t *bins, uint8_t *registers, uint32_t cap, uint32_t *n_sketched, uint32_t *n_dropped_bins, int reset);

/* ---- hot path --------------------------------------------------------------------------------- */
/* Replaces: the kt_forpool fan-out in classify_seqs (classifier.h:275) over classify_seq
 * (classifier.h:212-251), i.e. per read (or mate pair): Encoder::for_each -> kh_get(c) ->
 * linear::counter -> resolve_tree.
 *   bases    concatenated ASCII sequences (bseq1_t::seq, kseq_declare.h:40-44), no terminators needed
 *   offsets  n_reads+1 byte offsets into bases
 *   paired   0: one unit per read; 1: reads 2u,2u+1 are mates (one vote per pair, classifier.h:233-236)
 * Outputs, one entry per unit (n_reads or n_reads/2):
 *   taxon    resolve_tree result (0 = unclassified)
 *   missing  k-mers absent from the table                      (classifier.h:227)
 *   ambig    the reference's u32 ambig_count arithmetic        (classifier.h:232,235)
 *   n_hits   hits (taxa.size()); may be NULL
 *   hits     optional (NULL to skip): ordered hit taxids = the reference's `taxa` vector
 *            (classifier.h:228), unit u's hits start at hits[offsets[first read of u]]; array has
 *            offsets[n_reads] entries. */
int bns_classify_batch(bns_ctx *ctx, const char *bases, const uint64_t *offsets, uint64_t n_reads,
                       int paired, uint32_t *taxon, uint32_t *missing, uint32_t *ambig,
                       uint32_t *n_hits, uint32_t *hits);
/* Same call with the hit stream returned run-length encoded -- exactly what the Kraken formatter prints
 * (append_taxa_runs / classifier.h:45-61: "taxid:count" per run of equal consecutive hits), computed on the device so that
 * 4 bytes per k-mer do not cross PCIe.  Unit u's runs are run_tax[run_start[u] + j], run_len[run_start[u] + j] for
 * j < n_runs[u]; run_tax / run_len point into buffers owned by the context (valid until the next call on it), holding
 * *n_runs_total entries.  Where a unit's runs sit in them may differ from call to call; their content does not. */
int bns_classify_batch_runs(bns_ctx *ctx, const char *bases, const uint64_t *offsets, uint64_t n_reads, int paired,
                            uint32_t *taxon, uint32_t *missing, uint32_t *ambig, uint32_t *n_hits, uint64_t *run_start,
                            uint32_t *n_runs, const uint32_t **run_tax, const uint32_t **run_len, uint64_t *n_runs_total);
/* Device-resident variant: every pointer is a device pointer; max_read_len is the caller's upper
 * bound on any read length in the batch (0 = unknown: the call measures it, costing one sync).
 * d_bases must be 4-byte aligned and readable up to the next 4-byte boundary past total_bases (any hipMalloc'd or
 * framework-allocated buffer is). */
int bns_classify_batch_device(bns_ctx *ctx, const char *d_bases, const uint64_t *d_offsets,
                              uint64_t n_reads, uint64_t total_bases, uint32_t max_read_len, int paired,
                              uint32_t *d_taxon, uint32_t *d_missing, uint32_t *d_ambig,
                              uint32_t *d_n_hits, uint32_t *d_hits, void *stream);

/* ---- packed reads (north_star: "reads batched and packed 2-bit into coalesced HBM loads"; SURVEY 8b's proposed
 * classify_batch(ctx, packed_bases, valid_mask, read_offsets, ...)) ------------------------------------------------------------------
 * The same batch as above in the form the kernel works on: 2-bit codes A0 C1 G2 T3 (alphabet.h:128), 32 bases per uint64_t
 * word, FIRST base in the TOP two bits (the reference's own k-mer bit order, encoder.h:255: a k-mer is a funnel shift of two
 * adjacent words).  offsets[] are still base offsets; read r's words start at word (offsets[r] >> 5) + r (monotone, never
 * overlapping, no prefix sum needed) and the whole batch takes bns_packed_words(total_bases, n_reads) words.  Bases that are not
 * A/C/G/T (N, IUPAC, ...; their code bits are ignored) are flagged per word: bit (31 - i) of the word's 32-bit flag word = base
 * i of that word is invalid.  40 bytes per 150-bp read cross PCIe and HBM instead of 150.
 *   bns_pack_reads            host: ASCII batch -> words + the SPARSE list (word index, flags) of the words that hold an invalid
 *                             base (AVX2/BMI2 when the CPU has them; `threads` workers).  *n_bad = entries written; when it
 *                             exceeds bad_cap nothing is stored there and BNS_ERR_ARG comes back with *n_bad = the room needed.
 *   bns_pack_reads_ptrs       the same from reads that are NOT contiguous in memory (seqs[r], lens[r]: e.g. bseq1_t::seq of a chunk,
 *                             kseq_declare.h:40-44): fills offsets[n_reads + 1] itself -- packing replaces the gather copy a host
 *                             would otherwise make.
 *   bns_classify_batch_packed / _packed_runs   host buffers, as bns_classify_batch / _runs; the flags travel as the sparse list
 *                             (n_bad may be 0) and are scattered into a dense array on the device.
 *   bns_classify_batch_packed_device          everything resident; d_nmask = one flag word per packed word (dense), or NULL when
 *                             no read of the batch holds an invalid base.
 * Replaces the same reference code as bns_classify_batch (classifier.h:212-251); results are identical for the same reads. */
uint64_t bns_packed_words(uint64_t total_bases, uint64_t n_reads);
int bns_pack_reads(const char *bases, const uint64_t *offsets, uint64_t n_reads, uint64_t *words, uint64_t *bad_word,
                   uint32_t *bad_mask, uint64_t bad_cap, uint64_t *n_bad, int threads);
int bns_pack_reads_ptrs(const char *const *seqs, const uint32_t *lens, uint64_t n_reads, uint64_t *offsets, uint64_t *words,
                        uint64_t *bad_word, uint32_t *bad_mask, uint64_t bad_cap, uint64_t *n_bad, int threads);
/* (version 108) bns_pack_reads_ptrs with a quality string per read: quals[r] has lens[r] bytes, or is NULL (a read without quality;
 * quals itself may be NULL).  A base whose quality byte is below 33 + min_quality (unsigned; min_quality in [0, 93], else BNS_ERR_ARG) is
 * flagged like an invalid base and its code bits are 0 -- the image bns_pack_reads_ptrs makes of the same reads with 'N' in those places.
 * min_quality = 0: bns_pack_reads_ptrs. */
int bns_pack_reads_qual_ptrs(const char *const *seqs, const char *const *quals, const uint32_t *lens, uint64_t n_reads, uint32_t min_quality,
                             uint64_t *offsets, uint64_t *words, uint64_t *bad_word, uint32_t *bad_mask, uint64_t bad_cap, uint64_t *n_bad,
                             int threads);
int bns_classify_batch_packed(bns_ctx *ctx, const uint64_t *words, const uint64_t *bad_word, const uint32_t *bad_mask, uint64_t n_bad,
                              const uint64_t *offsets, uint64_t n_reads, int paired,
                              uint32_t *taxon, uint32_t *missing, uint32_t *ambig, uint32_t *n_hits, uint32_t *hits);
int bns_classify_batch_packed_runs(bns_ctx *ctx, const uint64_t *words, const uint64_t *bad_word, const uint32_t *bad_mask, uint64_t n_bad,
                                   const uint64_t *offsets, uint64_t n_reads, int paired,
                                   uint32_t *taxon, uint32_t *missing, uint32_t *ambig, uint32_t *n_hits, uint64_t *run_start,
                                   uint32_t *n_runs, const uint32_t **run_tax, const uint32_t **run_len, uint64_t *n_runs_total);
int bns_classify_batch_packed_device(bns_ctx *ctx, const uint64_t *d_words, const uint32_t *d_nmask, const uint64_t *d_offsets,
                                     uint64_t n_reads, uint64_t total_bases, uint32_t max_read_len, int paired, uint32_t *d_taxon,
                                     uint32_t *d_missing, uint32_t *d_ambig, uint32_t *d_n_hits, uint32_t *d_hits, void *stream);

/* Replaces: Encoder<score::Lex,u64>::for_each(func, str, len) (encoder.h:415-442) over a batch; also
 * what python/bns.cpp from_str/seqlist return (python/bns.cpp:87-129).  kmers has offsets[n_reads]
 * entries; read r's k-mers start at kmers[offsets[r]], n_kmers[r] of them, in sequence order. */
int bns_encode_batch(bns_ctx *ctx, const char *bases, const uint64_t *offsets, uint64_t n_reads,
                     uint64_t *kmers, uint32_t *n_kmers);
int bns_encode_batch_device(bns_ctx *ctx, const char *d_bases, const uint64_t *d_offsets, uint64_t n_reads,
                            uint64_t total_bases, uint64_t *d_kmers, uint32_t *d_n_kmers, void *stream);

/* Replaces: RollingHasher<uint64_t>(k, canon)::for_each_hash(func, s, l) without a window (encoder.h:644-865: canonical
 * path :692-760, other :762-796; CyclicHash rollinghash/cyclichash.h:23-154), as python/bns.cpp:42-77 uses it.  One 64-bit
 * value per k-window of every run of A/C/G/T the reference's loop visits (an invalid character skips k + 1 characters and
 * restarts; the canonical path stops when fewer than 2k characters remain after it), in order; sequence r's values start at
 * hashes[offsets[r]], n_hashes[r] of them.  The 256-entry character tables are an INPUT: the reference draws them from
 * wy::WyRand, a third-party generator absent from its checkout (parity unpinned); NULL, NULL = tables from
 * bns_rolling_tables(1337, 137, ...), the constructor's default seeds through a restated generator. */
int bns_rolling_hash_batch(bns_ctx *ctx, const char *bases, const uint64_t *offsets, uint64_t n_seqs, uint32_t k, int canon,
                           const uint64_t *fwd_table, const uint64_t *rc_table, uint64_t *hashes, uint32_t *n_hashes);
/* Replaces: RollingHasher<uint64_t>(k, canon, DNA, w) -- the same hasher with a window (encoder.h:664-671; windowed branches
 * :706-736 and :771-795): every hash goes through a QueueMap of w-k+1 entries scored by lex_score (FRev64) and the
 * minimum by (score, value) comes out once the queue is full; the canonical path queues BOTH strands' hashes (forward, then
 * reverse) as separate entries; the queue survives a restart at an invalid character; a sequence that never fills it yields
 * one value.  w <= k: no window (bns_rolling_hash_batch).  Layout: with P = 2 for (w > k and canon) else 1, hashes must hold
 * P * offsets[n_seqs] values and sequence r's values start at hashes[P * offsets[r]], n_hashes[r] of them. */
int bns_rolling_hash_windowed_batch(bns_ctx *ctx, const char *bases, const uint64_t *offsets, uint64_t n_seqs, uint32_t k, int canon,
                                    uint32_t w, const uint64_t *fwd_table, const uint64_t *rc_table, uint64_t *hashes,
                                    uint32_t *n_hashes);
/* The default tables: 256 + 256 values seeded the way encoder.h:682-683 seeds the forward / reverse hashers. */
int bns_rolling_tables(uint64_t seed1, uint64_t seed2, uint64_t *fwd, uint64_t *rc);
/* Replaces: RollingHasher<__uint128_t, CyclicHash<__uint128_t>>(k, canon)::for_each_hash(func, s, l) (encoder.h:644-865 with a
 * 128-bit word; the instantiation test/encoding.cpp:152 constructs) without a window: the same visiting rules as
 * bns_rolling_hash_batch, 128-bit rotations, myr = k % 128.  Every value and every table entry is a (lo, hi) pair of u64:
 * tables hold 256 entries = 512 u64, hashes_lohi must hold 2 * offsets[n_seqs] u64 and sequence r's values start at
 * hashes_lohi[2 * offsets[r]].  NULL, NULL = the constructor's default seeds through the restated generator, including
 * CharacterHash<u128>'s habit of keeping only the low word of each entry (characterhash.h:82-97).  Parity unpinned as for the
 * 64-bit hasher.
 * bns_rolling_hash128_windowed_batch: the same hasher with a window, RollingHasher<__uint128_t>(k, canon, DNA, w) -- the form the
 * reference's one RollingHasher test constructs (test/encoding.cpp:152-156; window branches encoder.h:706-736, 771-795): a
 * QueueMap of w - k + 1 entries, minimum by (score, value), both strands queued separately on the canonical path, the queue
 * surviving restarts, one flushed value for a stream that never fills it.  The queue's score is lex_score(u128) =
 * sketch::hash::CEHasher in the reference (un-vendored: restated as FRev64 over the folded halves, parity unpinned); the COUNT of
 * values -- what that test pins: len - w + 1 -- does not depend on it.  Layout: P = 2 for (w > k and canon) else 1; hashes_lohi
 * holds 2 * P * offsets[n_seqs] u64, sequence r's values start at hashes_lohi[2 * P * offsets[r]].  Not built: RollingHasherSet. */
int bns_rolling_hash128_batch(bns_ctx *ctx, const char *bases, const uint64_t *offsets, uint64_t n_seqs, uint32_t k, int canon,
                              const uint64_t *fwd_lohi, const uint64_t *rc_lohi, uint64_t *hashes_lohi, uint32_t *n_hashes);
int bns_rolling_hash128_windowed_batch(bns_ctx *ctx, const char *bases, const uint64_t *offsets, uint64_t n_seqs, uint32_t k, int canon,
                                       uint32_t w, const uint64_t *fwd_lohi, const uint64_t *rc_lohi, uint64_t *hashes_lohi,
                                       uint32_t *n_hashes);
int bns_rolling_tables128(uint64_t seed1, uint64_t seed2, uint64_t *fwd_lohi, uint64_t *rc_lohi);

/* Replaces: Encoder<>::for_each_hash(func, str, len, k = 0) (encoder.h:355-394) -- the ntHash stream of a contiguous,
 * unwindowed seed, as bin/kmercnt.cpp:78, bin/setsketcher.cpp:98,129-130 select it ("k > 32 implies nthash").  One value per
 * k-window the reference's loop visits: every window of every run of A/C/G/T (either case) at least k long, in order --
 * except that a run whose first window ends exactly at the end of the sequence yields nothing (the NUL test comes first at
 * encoder.h:378-379; so a sequence of exactly k bases is silent) and a NUL byte ends the sequence.  canon: 1 = NTC64's
 * canonical value min(forward, reverse), 0 = the forward value, -1 = the encoder's canonicalize flag (encoder.h:383,392).
 * k = 0 = the encoder's k; k may exceed 32 (the hash is 64-bit whatever k is).  A spaced or windowed encoder is refused as
 * encoder.h:363-364 does.  The arithmetic is NTC64 of bcgsc/ntHash, an un-vendored submodule (.gitmodules, version unpinned):
 * restated from the published definition (rol/ror form of ntHash 1.0.x) with the 256-entry seed table as an INPUT --
 * PARITY UNPINNED.  table256 follows make_nthash_lut's in-tree geometry (encoder.h:93-103: a base's seed at
 * its letter, its complement's seed at letter & 7); NULL = ntHash's published seeds.  Sequence r's values start at
 * hashes[offsets[r]], n_hashes[r] of them. */
int bns_for_each_hash_batch(bns_ctx *ctx, const char *bases, const uint64_t *offsets, uint64_t n_seqs, uint32_t k, int canon,
                            const uint64_t *table256, uint64_t *hashes, uint32_t *n_hashes);
int bns_nthash_tables(uint64_t seed_a, uint64_t seed_c, uint64_t seed_g, uint64_t seed_t, uint64_t *table256);

/* Replaces: kh_get(c, db, kmer) + kh_val (khash64.h:250-263) over a batch of keys.
 * found[i] = 1 and vals[i] = value on a hit; found[i] = 0, vals[i] = 0 on a miss. */
int bns_probe(bns_ctx *ctx, const uint64_t *kmers, uint64_t n, uint32_t *vals, uint8_t *found);
int bns_probe_device(bns_ctx *ctx, const uint64_t *d_kmers, uint64_t n, uint32_t *d_vals, uint8_t *d_found,
                     void *stream);

/* Replaces: resolve_tree(hit_counts, taxmap) (util.h:831-869) over a batch of counters given in
 * insertion order: unit u owns keys/counts[starts[u] .. starts[u+1]). */
int bns_resolve_batch(bns_ctx *ctx, const uint32_t *keys, const uint16_t *counts, const uint64_t *starts,
                      uint64_t n_units, uint32_t *taxon);

/* ---- database construction on device (feature_min.h:205-228 update_lca_map) ------ */
/* Builds khash_t(c) arrays (valid for kh_get and for bns.db) in HBM from n_genomes sequences:
 * every k-mer the encoder emits for genome g maps to taxid[g]; a k-mer seen under several taxids maps
 * to their lca().  n_buckets must be a power of two with load <= 0.77 (khash64.h:198).  Requires a
 * loaded taxonomy and encoder.  Outputs are device arrays sized like bns_load_table's inputs;
 * header4 (host) receives {n_buckets, n_occupied, size, upper_bound}. */
int bns_build_table_device(bns_ctx *ctx, const char *d_bases, const uint64_t *d_offsets, uint64_t n_genomes,
                           uint64_t total_bases, const uint32_t *d_taxid, uint64_t n_buckets,
                           uint32_t *d_flags, uint64_t *d_keys, uint32_t *d_vals, uint64_t *header4,
                           void *stream);

/* ---- build session (version 109): a table that persists in the context, grows, and can start from a bns.db -------------------
 * bns_build_table_device wants all sequences in one call and a table size guessed in advance.  A session takes them batch by
 * batch: the table lives in the context, doubles when a batch does not fit, and may be seeded from an existing khash table, so a
 * db can be extended with new genomes alone.  The stored value is the lca() of all contributing taxids and the fold is
 * order-free, so a seeded table plus new sequences is the table of a build over the union.
 *   bns_build_begin   needs a loaded taxonomy and encoder, refuses what bns_build_table_device refuses (k == 32 forward contiguous,
 *                     a spaced seed without spaced_intended), and allocates max(4, n_buckets_hint rounded up to a power of two)
 *                     empty buckets.  A second begin -- and bns_set_encoder, bns_set_window or bns_load_taxonomy while the session
 *                     is open -- returns BNS_ERR_STATE.
 *   bns_build_seed    host arrays in bns_load_table's form; once, between begin and the first add.  Every slot whose flag pair is 0
 *                     (present) goes in with its value as it is; empty AND deleted slots are skipped whatever their key and value
 *                     words hold.  The session table is first sized so that the seeded keys sit at a load <= 0.77.
 *   bns_build_add     one batch of whole sequences, the inputs of bns_build_table_device (device arrays; n_seqs + 1 offsets, the
 *                     bases readable 8 bytes past the end).  Inserts the batch's keys and folds its taxids into the values.  When
 *                     the table fills up, or more than 0.77 n_buckets keys are in, the table is doubled (rehashed on the device) and
 *                     the SAME batch applied again -- inserting and folding are idempotent --, until it fits; earlier batches are
 *                     never encoded again.  Returns when the device is done with the batch: the caller may free it.
 *   bns_build_finish  compacts to khash's own size (the smallest power of two nb >= 4 with (uint64_t)(nb * 0.77 + 0.5) >= size),
 *                     writes the flags, zeroes empty slots, and reports header4 = {n_buckets, n_occupied, size, upper_bound}.  A
 *                     session without a key finishes as a valid empty table of 4 buckets.
 *   bns_build_export  the finished arrays to the host, sized by header4 as bns_load_table's inputs are.
 *   bns_build_stats   out6 = {batches added, grows, keys seeded, keys in the table, microseconds of wall time inside bns_build_add so
 *                     far, the part of them spent growing} of the open session.
 *   bns_build_end     frees the session; legal at any point (no session: nothing happens).  bns_destroy ends an open session.
 * add / finish / export / seed / stats without a session, add after finish, export before finish and seed after an add return
 * BNS_ERR_STATE.
 * Memory: the table takes 12 bytes a bucket while it is built (12.25 finished).  A grow holds the old table and the new one side
 * by side, so growing from n to 2n buckets needs 36 n bytes for a moment.  A grow that cannot be allocated returns BNS_ERR_TABLE
 * with a message and faults nothing; after it -- as after any failed add -- the session holds keys without their values and
 * accepts bns_build_end only. */
int bns_build_begin(bns_ctx *ctx, uint64_t n_buckets_hint);
int bns_build_seed(bns_ctx *ctx, uint64_t n_buckets, const uint32_t *flags, const uint64_t *keys, const uint32_t *vals);
int bns_build_add(bns_ctx *ctx, const char *d_bases, const uint64_t *d_offsets, uint64_t n_seqs, uint64_t total_bases,
                  const uint32_t *d_taxid, void *stream);
int bns_build_finish(bns_ctx *ctx, uint64_t *header4);
int bns_build_export(bns_ctx *ctx, uint32_t *flags, uint64_t *keys, uint32_t *vals);
int bns_build_stats(const bns_ctx *ctx, uint64_t *out6);
int bns_build_end(bns_ctx *ctx);

/* ---- taxonomic-depth minimizers (version 111): the session's table thinned by the deepest LCA of every window -------------------
 * A session that has added every sequence with the window unset holds F: every k-mer -> the lca() of all sequences holding it.
 * Minimizing streams the SAME sequences a second time.  Sequence s of n bases has max(0, n - w + 1) windows; window p holds the
 * k-mers that start at p .. p + w - c (c = the comb).  With depth(t) = nodes on the chain t -> root, root included (0 for
 * 0xFFFFFFFF, for an id that is no node and for a chain that reaches no root) and score(x) = (0xFFFFFFFF - depth(F[x])) << 32 | F[x],
 * a window selects, among its valid k-mers (every sampled base A/C/G/T in either case; a spaced all-T 32-mer is not valid), the one
 * with the smallest (score, k-mer): the deeper LCA, then the smaller taxid, then the smaller k-mer.  A window without a valid
 * k-mer and a sequence shorter than w select nothing; w <= c selects every valid k-mer.  The table M holds every selected k-mer
 * with the value F holds for it; it is a function of the set of sequences, whatever the batches, their order and the sizes.
 *   bns_build_minimize_begin  in an open, unfinished, unfailed session whose window is not beyond the comb (else BNS_ERR_STATE; a
 *                             second begin too).  Refuses w > 1920 and w - c + 1 > 1024 (BNS_ERR_ARG).  Freezes F -- bns_build_add
 *                             and bns_build_seed return BNS_ERR_STATE from here on --, computes the depth of every taxonomy node on
 *                             the device and allocates M with max(4, n_buckets_hint rounded up to a power of two) buckets.
 *   bns_build_minimize_add    bns_build_add's inputs without taxids.  One lookup in F per valid position and 2048-base chunk; M
 *                             doubles as the session table does, and the same batch is applied again (idempotent).  A k-mer that F
 *                             does not hold fails the call with BNS_ERR_TABLE ("not part of the scored build") and faults nothing.
 *                             Returns when the device is done with the batch.  After a failed call only bns_build_end is accepted.
 *   bns_build_minimize_stats  out6 = {batches, grows of M, keys in F, keys in M, positions looked up, microseconds inside add}.
 * After bns_build_minimize_begin, bns_build_finish / bns_build_export act on M (khash's own size, flags, empty slots zeroed) and
 * bns_build_stats' "keys in the table" counts M's; F is freed by bns_build_end.  Memory: 12 bytes a bucket for F and for M, 4 bytes a
 * taxonomy node for the depths; a grow of M holds two copies of M beside F.  minimize_add before minimize_begin, and either after
 * bns_build_finish or without a session, return BNS_ERR_STATE. */
int bns_build_minimize_begin(bns_ctx *ctx, uint32_t w, uint64_t n_buckets_hint);
int bns_build_minimize_add(bns_ctx *ctx, const char *d_bases, const uint64_t *d_offsets, uint64_t n_seqs, uint64_t total_bases,
                           void *stream);
int bns_build_minimize_stats(const bns_ctx *ctx, uint64_t *out6);

/* ---- fewest-genome minimizers (version 114): every window keeps the k-mer that the fewest genomes hold ----------------------------
 * Every sequence carries a genome id, a u32 below 0xFFFFFFFF (`bonsai build -G`: the index of its file).  n(x) is the number of
 * DISTINCT genome ids among the sequences that hold x as a valid k-mer: a k-mer that occurs five times in one genome, in one contig
 * or in several, has n = 1.  With score(x) = (n(x) << 32) | F[x] a window selects the smallest (score, k-mer): fewer genomes, then
 * the smaller taxid, then the smaller k-mer; windows, validity, w <= c and M's values (F[k-mer]) are those of the section above.  M is
 * a function of the set of (sequence, genome id, taxid) triples: batch cuts, table sizes and grows change nothing, nor does the
 * numbering of the ids so long as it keeps the partition of the sequences.
 * The counts are a third stream of the SAME sequences, between the adds and the minimizing:
 *   bns_build_count_begin   in an open, unfinished, unfailed session whose window is not beyond the comb and that is not minimizing
 *                           (else BNS_ERR_STATE; a second begin too).  Freezes F -- bns_build_add and bns_build_seed return
 *                           BNS_ERR_STATE from here on -- and allocates a zeroed count and stamp per bucket of F: no memory for them
 *                           is BNS_ERR_TABLE, and the session stays as it was.
 *   bns_build_count_add     bns_build_minimize_add's inputs plus a HOST array of n_seqs genome ids.  The ids must not decrease within
 *                           the call, the first must be at least the last id of the previous call, none may be 0xFFFFFFFF: otherwise
 *                           BNS_ERR_ARG with nothing enqueued and nothing changed.  One kernel launch per run of equal ids (a genome is
 *                           counted once because every lane in flight carries ONE id: count_kernel, csrc/bns_fewest.hpp).  A k-mer that
 *                           F does not hold fails the call with BNS_ERR_TABLE ("not part of the scored build") and faults nothing;
 *                           after that only bns_build_end is accepted.  n_seqs == 0 counts as a batch.  Returns when the device is
 *                           done with the batch.
 *   bns_build_count_get     n(x) so far for n keys as the encoder emits them (host arrays), 0 for a key F does not hold.  From
 *                           bns_build_count_begin until bns_build_end, also after bns_build_minimize_begin and bns_build_finish
 *                           behind it; on the context's own stream.  (A bns_build_finish WITHOUT minimizing compacts the table the
 *                           counts belong to: BNS_ERR_STATE from then on.)
 *   bns_build_count_stats   out6 = {batches, launches (genome runs), distinct genome ids seen, positions looked up, the largest count,
 *                           microseconds inside add}.
 *   bns_build_minimize_begin_score  bns_build_minimize_begin with the score named: BNS_MINIMIZE_DEPTH is that call as it is;
 *                           BNS_MINIMIZE_FEWEST needs bns_build_count_begin to have been called (else BNS_ERR_STATE), computes no
 *                           depths and selects by the counts as they stand.  Any other score: BNS_ERR_ARG.
 * Memory: 8 more bytes a bucket of F from bns_build_count_begin to bns_build_end. */
#define BNS_MINIMIZE_DEPTH 0
#define BNS_MINIMIZE_FEWEST 1
int bns_build_count_begin(bns_ctx *ctx);
int bns_build_count_add(bns_ctx *ctx, const char *d_bases, const uint64_t *d_offsets, uint64_t n_seqs, uint64_t total_bases,
                        const uint32_t *h_genome, void *stream);
int bns_build_count_get(bns_ctx *ctx, const uint64_t *h_keys, uint64_t n, uint32_t *h_counts);
int bns_build_count_stats(const bns_ctx *ctx, uint64_t *out6);
int bns_build_minimize_begin_score(bns_ctx *ctx, uint32_t w, uint64_t n_buckets_hint, int score);

/* ---- window session (version 110): every window of L bases of every sequence, called as a read (`bonsai distrib`) -------------
 * With L = window_len, sequence s of n bases has max(0, n - L + 1) windows; window p is its bases [p, p + L).  The CALL of a window is
 * the taxon bns_classify_batch returns for that substring as a single unpaired read on this context -- its table layout, encoder
 * (canonical or not; a spaced seed without spaced_intended emits nothing, so every call is 0), taxonomy, and classify's handling of N,
 * other bytes and lower case -- bit for bit.  Each k-mer of a batch is looked up once, not once per window that holds it.
 *   bns_windows_begin  needs a loaded table, encoder and taxonomy, and no confidence threshold (bns_set_confidence), else
 *                      BNS_ERR_STATE; a second begin: BNS_ERR_STATE.  window_len must be at least the seed's span c, and
 *                      window_len - c + 1 <= 65535 (the vote's counts are 16 bits wide, as the reference's: inside the bound none can
 *                      wrap), else BNS_ERR_ARG.  pair_cap slots of the pair table, rounded up to a power of two; 0: BNS_ERR_ARG.  The
 *                      table starts empty.
 *   bns_windows_begin_conf (version 112)  bns_windows_begin with a confidence threshold theta = num / den that belongs to the SESSION
 *                      (argument rules of bns_set_confidence: den == 0 or num > den is BNS_ERR_ARG; num == 0 opens exactly the
 *                      session bns_windows_begin opens).  The call of a window is then the taxon bns_classify_batch returns for that
 *                      substring with bns_set_confidence(num, den) on, bit for bit: Q = the window's hits + looked-up-and-missing
 *                      k-mers (k-mers over an N do not enter, as `ambig` does not in classify), R = ceil(theta Q) exactly, and the
 *                      call T becomes the first of T, parent(T), ... whose clade (Euler interval, counted exactly) holds >= R of the
 *                      window's hits; 0 when hits < R or the walk passes a root; T stays when R = 0, T = 0 or T is no node whose chain
 *                      reaches a root.  Pair table, d_taxon image, n_dropped and bns_windows_read are as without a threshold; the walk
 *                      is part of the vote stage of bns_windows_timing.  The context's own threshold (bns_set_confidence) is never
 *                      inherited and, while on, still makes begin, begin_conf and add return BNS_ERR_STATE.
 *   bns_windows_add    one batch of whole sequences, bns_build_add's inputs (device arrays; n_seqs + 1 offsets, the bases readable
 *                      8 bytes past the end, a taxid per sequence).  d_taxon may be NULL; else it has total_bases entries: the call of
 *                      window p of sequence s goes to d_taxon[offsets[s] + p] (the convention of `hits`), and every base that starts no
 *                      window -- the last L - 1 of a sequence, all of a sequence shorter than L -- gets 0xFFFFFFFF.  Every window adds 1
 *                      to the count of the pair (d_taxid[s], call), calls of 0 included.  A pair that finds no free slot adds to
 *                      n_dropped instead: the pairs in the table are always exact, the sum of their counts plus n_dropped is the
 *                      number of windows added, and which pairs get in when the table is full is not defined.  (The pair
 *                      (0xFFFFFFFF, 0xFFFFFFFF) -- BNS_TAX_ABSENT as a sequence's taxid -- is always dropped.)  The work is queued
 *                      on `stream` (NULL: the context's) and the call returns: the batch and d_taxon are the device's until that
 *                      stream has been waited for.  A confidence threshold set since begin: BNS_ERR_STATE.
 *   bns_windows_read   waits for the device, then the pairs ascending by (seq_taxid, called); any of the three arrays may be NULL.
 *                      cap < *n_pairs: BNS_ERR_ARG with *n_pairs set (bns_sketch_read's rule).  reset empties the table and zeroes
 *                      n_dropped.
 *   bns_windows_timing a session begun while bns_set_timing is on brackets the three stages of every add with events -- packing the
 *                      bases and clearing the outputs | the lookup pass | the vote pass -- and WAITS for the batch at the end of the
 *                      add; ms3 receives the milliseconds summed over the *n_adds adds since the last call.  A session begun with
 *                      timing off: BNS_ERR_STATE.
 *   bns_windows_end    frees the session; legal at any point.  bns_destroy ends an open session.
 * add, read or timing without a session: BNS_ERR_STATE.  begin while bns_set_dust or bns_set_min_hit_groups is on: BNS_ERR_STATE.  bns_set_min_base_quality does
 * not apply (sequences carry no quality); the bns_tally_enable tally and the sketches are not touched (as with bns_resolve_batch).
 * Without a session nothing is allocated or launched. */
int bns_windows_begin(bns_ctx *ctx, uint32_t window_len, uint32_t pair_cap);
int bns_windows_begin_conf(bns_ctx *ctx, uint32_t window_len, uint32_t pair_cap, uint64_t num, uint64_t den);
int bns_windows_add(bns_ctx *ctx, const char *d_bases, const uint64_t *d_offsets, uint64_t n_seqs, uint64_t total_bases,
                    const uint32_t *d_taxid, uint32_t *d_taxon, void *stream);
int bns_windows_read(bns_ctx *ctx, uint32_t *seq_taxid, uint32_t *called, uint64_t *count, uint64_t cap, uint64_t *n_pairs,
                     uint64_t *n_dropped, int reset);
int bns_windows_timing(bns_ctx *ctx, double *ms3, uint64_t *n_adds);
int bns_windows_end(bns_ctx *ctx);

/* ---- instrumentation -------------------------------------------------------------------------- */
/* HIP-event timing of the dominant kernel (classify_kernel / probe_kernel), recorded on the stream the
 * kernel is launched on.  bns_set_timing(ctx, 1) enables and clears.  bns_last_kernel_ms: most recent
 * launch (< 0 if none).  bns_timing_summary: sum and count over the launches recorded since the last
 * summary (ring of 64), waits for them, then clears. */
int   bns_set_timing(bns_ctx *ctx, int enabled);
float bns_last_kernel_ms(const bns_ctx *ctx);
int   bns_timing_summary(bns_ctx *ctx, double *sum_ms, int *count);

/* raw device memory helpers so non-HIP hosts (ctypes tests) can stage buffers */
/* Page-locked host memory: the host-buffer entry points (bns_classify_batch, ...) copy from / to pageable memory through
 * the runtime's staging buffers at roughly a third of the PCIe rate; buffers obtained here go at full rate. */
int bns_host_alloc(bns_ctx *ctx, size_t bytes, void **out);
/* ... and memory the HOST allocated (and touched), page-locked where it lies: registering 96 MiB of huge-page memory that is already
 * resident takes 0.5 ms where bns_host_alloc takes 15-45 ms (it allocates, faults in and pins under the runtime's lock, with every other
 * thread's calls waiting: the first 0.15 s of a BGZF file were five such slots, tools/micro/pin_bench.hip); copies from it run at
 * 44-50 GB/s against 57.  Nothing in the reference (its buffers are kseq's: klib/kseq.h:62-75). */
int bns_host_register(bns_ctx *ctx, void *p, size_t bytes);
int bns_host_unregister(bns_ctx *ctx, void *p);
int bns_host_free(bns_ctx *ctx, void *p);
int bns_dev_alloc(bns_ctx *ctx, size_t bytes, void **out);
int bns_dev_free(bns_ctx *ctx, void *p);
int bns_dev_upload(bns_ctx *ctx, void *dst, const void *src, size_t bytes);
int bns_dev_download(bns_ctx *ctx, void *dst, const void *src, size_t bytes);
int bns_dev_sync(bns_ctx *ctx);

/* ---- FASTA / FASTQ text parsed on the device (host ingest) -------------------------------------------------------
 * Replaces: kseq_read (klib/kseq.h:177-225) + bseq_read's loop (kseq_declare.h:112-145) + the chunk's classify_seqs fan-out
 * (classifier.h:269-287) for text that is handed over AS TEXT: record boundaries, names, sequence lengths and the 2-bit words the
 * classify kernel reads are made by kernels from the raw bytes of the file -- uploaded from a read(2) buffer, or already in HBM
 * (BNS_TEXT_DEVICE: e.g. left there by bns_inflate_members_device) -- so neither a host parser nor a host packer is on the path.
 *   text[s], text_bytes[s]   n_streams = 1: one file's bytes; 2: a pair of files, record i of stream 0 and record i of stream 1 are
 *                            mates (kseq_declare.h:116-131).  text[s][0] must be the first byte of a record (or of the file).
 *   limit                    records of stream 0 that START at or behind this offset are left alone (a stretch of a file handed to
 *                            this device: the record that straddles its nominal end is this call's, the one that starts behind it
 *                            the next stretch's); >= text_bytes[0]: no limit
 *                            Device text (BNS_TEXT_DEVICE) may start at any address; it must be readable from the 64-byte boundary in front of it to
 *                            the 64-byte boundary behind its end.
 *   flags                    BNS_TEXT_FINAL: the text ends the input (kseq's end-of-file rules close the last record); otherwise the
 *                            last record that STARTS in the text is never taken (a FASTA record ends at the next header) -- it is
 *                            where consumed[] points.  BNS_TEXT_TRIM_READNO: trim_readno (kseq_declare.h:106-110) on every name.
 *   cap_records, out         room in the caller's arrays, in records.  Per unit (record; pair when n_streams = 2): taxon, missing,
 *                            ambig, n_hits as bns_classify_batch; run_start / n_runs as bns_classify_batch_runs (NULL: no runs).
 *                            Per record, mates interleaved: seq_len; rec_pos (offset of the record's header line in its text[s]);
 *                            names[name_off[r] .. name_off[r + 1]) = kseq's name field (first token of the header line).  Any
 *                            pointer but taxon may be NULL.
 *   info                     n_records taken (all streams together); consumed[s] = offset of the first byte of text[s] NOT taken:
 *                            the caller's next call starts there.  status:
 *     BNS_TEXT_OK            everything up to consumed[] was classified
 *     BNS_TEXT_IRREGULAR     the text at consumed[] is not in the form the kernels parse (below): that stretch is the host parser's
 *     BNS_TEXT_NO_RECORD     no complete record starts in what is left (a record longer than the text handed over)
 *     BNS_TEXT_CAP           the caller's arrays are full; call again from consumed[]
 * The REGULAR FORM (everything kseq_read parses the same way line by line; proof in docs/INGEST_NOTES.md): records are a header line
 * ('>' or '@' first) / sequence lines (first byte none of '>', '@', '+'; blank lines skipped) / optionally a '+' line and quality
 * lines -- one or several, whatever they start with -- that are together exactly as long as the sequence / blank lines; line ends
 * '\n' or '\r\n' (one trailing '\r' per appended line is dropped as ks_getuntil2 drops it, klib/kseq.h:135); at most 4096 lines per
 * record.  Wrapped FASTA, wrapped FASTQ sequences and quality (round 6), quality lines that start with '@' or '+', CRLF text (round 6),
 * a missing final newline, empty sequences are all regular; text between records and quality of the wrong length (kseq's error -2)
 * are not (status IRREGULAR: nothing is guessed).
 * Results are those of bns_classify_batch on the records kseq_read yields. */
#define BNS_TEXT_FINAL        1
#define BNS_TEXT_TRIM_READNO  2
#define BNS_TEXT_DEVICE       4
#define BNS_TEXT_PARSE_ONLY   8     /* records only (seq_len, rec_pos, names): nothing is classified; no table needed */
#define BNS_TEXT_DEFER        16    /* parse and pack now -- the call returns when the records are known: info->n_records, consumed[], status,
                                       why, total_bases, names_bytes; the caller's host buffers are his again -- and leave the classify launch, the
                                       hit runs and the copies of EVERY result array (seq_len, names, ... included) to bns_text_finish.  For a caller
                                       that hands blocks of one input to several devices in turn: where block b + 1 starts is known as soon as
                                       block b is parsed, so the next device parses while this one classifies (classifier.h:296-337 reads its
                                       chunks in order too; nothing here is guessed).  Until bns_text_finish the context takes no other
                                       bns_classify_text call (BNS_ERR_STATE; bns_text_prefetch is fine).  Not with out->words / nmask. */
#define BNS_TEXT_OK           0
#define BNS_TEXT_IRREGULAR    1
#define BNS_TEXT_NO_RECORD    2
#define BNS_TEXT_CAP          3
typedef struct bns_text_out {
    uint32_t *taxon, *missing, *ambig, *n_hits;      /* per unit */
    uint64_t *run_start; uint32_t *n_runs;           /* per unit; both or neither */
    uint32_t *seq_len; uint64_t *rec_pos;            /* per record */
    uint32_t *name_off; char *names; uint64_t names_cap;   /* name_off: cap_records + 1 entries */
    uint32_t *run_tax, *run_len; uint64_t runs_cap;  /* optional: where the hit runs go (entries; with run_start / n_runs).  NULL: buffers of the
                                                        context (info->run_tax / run_len, valid until its next call).  Too small: BNS_TEXT_CAP */
    uint64_t *words; uint32_t *nmask;                /* the records' 2-bit image, bns_pack_reads' layout with DENSE flag words
                                                        (bns_packed_words(total_bases, n_records) entries each): calls of one
                                                        piece only (<= 64 MiB of text per stream), BNS_ERR_ARG otherwise */
    /* (version 107; all zero: as before) The finished Kraken lines of the call's units, assembled by kernels from what is in HBM anyway --
     * name, length, result, hit runs -- instead of those ingredients coming back for a host formatter.  Replaces
     * append_kraken_classification (classifier.h:112-129, with append_taxa_runs / append_counts, classifier.h:45-70) and the kt_for loop that
     * formats a chunk (classifier.h:269-287).  lines[0, info->lines_bytes): the lines in unit order, contiguous across the call's batches;
     * a pair prints the first mate's name and length; a unit is printed when BNS_LINES_ALL is set or its taxon is not 0
     * (classifier.h:239).  line_off (optional; n_units + 1 entries, cap_records + 1 of room): unit u's line is lines[line_off[u],
     * line_off[u + 1]) -- empty for a unit that is not printed.  With lines the hit runs are computed whether or not run_start / n_runs are
     * given, and every other array but taxon stays optional.  lines_cap too small: BNS_TEXT_CAP, with n_records / consumed[] / lines_bytes
     * those of the batches whose lines fit whole (behind BNS_TEXT_DEFER: bns_text_finish then reports fewer records than the first half
     * did); call again from consumed[].  Not with BNS_TEXT_PARSE_ONLY (BNS_ERR_ARG). */
    char *lines; uint64_t lines_cap;                 /* page-locked or plain host memory */
    uint64_t *line_off;
    uint32_t lines_flags;                            /* BNS_LINES_* */
} bns_text_out;
#define BNS_LINES_ALL         1u    /* print unclassified units too (emit_all: `bonsai classify -a`) */
typedef struct bns_text_info {
    uint64_t n_records, consumed[2], total_bases, names_bytes, n_runs_total;
    const uint32_t *run_tax, *run_len;               /* owned by the context, valid until its next call */
    int32_t status;
    uint32_t why;                                    /* IRREGULAR: BNS_TEXT_WHY_* bits of the first offending stretch */
    uint32_t n_slices, n_launches;                   /* parses (one per upload piece, and more where a window filled up) / classify launches (one per ~2 M records) */
    double ms_parse, ms_classify;                    /* device time of the parse kernels / of classify (HIP events; bns_set_timing) */
    uint64_t lines_bytes;                            /* (version 107) bytes written to out->lines */
    double ms_lines;                                 /* out->lines: hit runs, line lengths, the read-back of the batch's byte count and the line
                                                        bytes, first kernel to last (HIP events; bns_set_timing) */
} bns_text_info;
#define BNS_TEXT_WHY_CR          1u    /* (round 5: a line ends in '\r'.  Round 6 reads CRLF text on the device: not reported any more) */
#define BNS_TEXT_WHY_LEADING     2u    /* text in front of the first header */
#define BNS_TEXT_WHY_AFTER_QUAL  4u    /* a sequence or '+' line where only a header or a blank line may stand */
#define BNS_TEXT_WHY_QUAL_LEN    8u    /* the quality lines do not end where they are as long as the sequence (kseq's error -2: too long, or the input ends first) */
#define BNS_TEXT_WHY_PLUS_RUN    16u   /* (round 5: more than 16 consecutive lines that start with '+'.  Not reported any more: quality may span lines) */
#define BNS_TEXT_WHY_LONG_RECORD 32u   /* more than 4096 lines in one record */
#define BNS_TEXT_WHY_LINES       64u   /* more lines than one per 8 bytes of text (+ 1024), or more lines that start with '>' / '@' than one per 16 bytes (+ 512) */
int bns_classify_text(bns_ctx *ctx, const char *const *text, const uint64_t *text_bytes, int n_streams, uint64_t limit, int flags,
                      uint64_t cap_records, const bns_text_out *out, bns_text_info *info);
/* Optional: start the upload of the text of the NEXT bns_classify_text call now, so that it travels while the current call
 * computes (a call uploads its own text in pieces and overlaps them with ITS compute; what it cannot overlap is its first piece and
 * its last piece's compute -- a host that calls `prefetch(block b + 1); classify(block b)` keeps the link busy across calls).
 * Returns at once.  The next call's text[s] may be any sub-range of what was prefetched (a block whose first record's offset is
 * only known when the block in front is done); text that was not prefetched is uploaded by the call as before.  The host buffers
 * must stay untouched until the call that consumes them returns; at most one prefetch may be outstanding beside the text of the
 * call in progress (BNS_ERR_STATE otherwise).  n_streams = 0 (text, text_bytes ignored): wait for uploads in flight and forget them --
 * a caller that gives its buffers up without the call that would have consumed them (an input that ended early, an error). */
int bns_text_prefetch(bns_ctx *ctx, const char *const *text, const uint64_t *text_bytes, int n_streams);
/* The second half of a bns_classify_text(..., BNS_TEXT_DEFER, ...) call: classifies what that call parsed, fills the result arrays it was
 * given (they must still be there) and `info` like a call without the flag would have.  status BNS_TEXT_CAP with fewer records than the
 * first half reported: the caller's run arrays were too small -- call bns_classify_text again on the same text with larger ones (the records
 * and consumed[] will be the same).  Replaces nothing in the reference: its classify_seqs (classifier.h:269-287) returns when a chunk is done. */
int bns_text_finish(bns_ctx *ctx, bns_text_info *info);
/* ---- minimum base quality (what `bonsai classify -Q` sets; version 108) ---------------------------------------------------------
 * No reference counterpart: Kraken 2's --minimum-base-quality, as defined in DESIGN.md.  q in [0, 93], Phred+33.  For a record that has
 * quality (kseq_read returned a quality string: a '+' line), base i of the sequence is MASKED when byte i of the quality string -- both as
 * kseq_read yields them -- is below 33 + q, unsigned.  A masked base is an invalid base: its flag is set and its code bits are 0 in the
 * packed image, so every k-mer over it is skipped like one over an 'N'; missing, ambig, the hits, runs, lines, the tally and the
 * confidence walk follow from the image.  FASTA records are untouched.  Only flags change: seq_len, names, rec_pos, consumed[], status and
 * why are those of the same call with q = 0.  bns_classify_text applies it while it packs (pack_text_minq_kernel: the quality bytes are
 * gathered beside the bases from text that lies in HBM already), so behind BNS_TEXT_DEFER it is the first half's setting that counts;
 * out->words / out->nmask hold the masked image.  Per context; table and taxonomy reloads keep it.  q > 93: BNS_ERR_ARG.  q = 0 turns it
 * off (the default): nothing is launched, allocated or read that was not before.  bns_classify_batch* take no quality: a caller that holds
 * one masks with bns_pack_reads_qual_ptrs. */
int bns_set_min_base_quality(bns_ctx *ctx, uint32_t q);
/* ---- low-complexity masking (what `bonsai classify -m` and `bonsai build -m` set; version 113) ------------------------------------
 * No reference counterpart: the step Kraken 2 applies to a library before it builds (dustmasker / k2mask), as symmetric DUST (Morgulis et
 * al. 2006) defined in DESIGN.md.  window W in [8, 64] bases, level T in [1, 1000] (dustmasker's defaults: 64, 20).  Inside a maximal run
 * of valid bases of one sequence -- valid as the packed image flags it: an N, any other byte and a base below bns_set_min_base_quality end a
 * run -- a triplet is three consecutive bases; an interval of l consecutive triplets, 2 <= l <= W - 2, scores S = sum over triplet values
 * t of c_t (c_t - 1) / 2, over (l - 1), c_t the occurrences of t in the interval; it is PERFECT when 10 S > T and no sub-interval (l >= 2)
 * scores strictly higher; the mask is the union of the bases of all perfect intervals (l + 2 bases each).  Exact integer cross-products,
 * no floating point.  A masked base is an invalid base: its flag is set and its code bits are 0, exactly what a minimum base quality does
 * to a base, and everything behind the image follows from it.  No reverse-complement symmetry and no parity with NCBI dustmasker or
 * minimap2's sdust is claimed.
 * While on: every classifying entry point (those bns_tally_enable lists) packs ASCII input first (pack_kernel), masks the image
 * (dust_mark_kernel, dust_apply_kernel on the call's stream) and classifies in the packed form; a caller's packed image is never written:
 * a copy in the context's workspace is masked.  bns_classify_text masks behind its pack (quality masking first), and out->words /
 * out->nmask hold the masked image.  bns_build_table_device, bns_build_add and bns_build_minimize_add mask the sequences they are given
 * (both passes of a depth-minimizer build see the same mask).  bns_encode_batch*, the hash feeders, bns_probe* and bns_resolve_batch are
 * not affected.  bns_windows_begin* return BNS_ERR_STATE while it is on: a window's call is classify's call of that substring as a read,
 * and the mask of a substring is not the genome's mask restricted to it.
 * window = 0 turns it off (the default; level is ignored): nothing is launched, allocated or read that was not before.  Otherwise window
 * outside [8, 64] or level outside [1, 1000]: BNS_ERR_ARG.  While a build or window session is open: BNS_ERR_STATE.  Per context; table
 * and taxonomy reloads keep it.  A db does not record that it was built masked: the caller has to remember.
 * bns_dust_mask: the mask alone, for host arrays (bases, n_seqs + 1 offsets) with the context's current window and level; flags receives
 * bns_packed_words(offsets[n_seqs], n_seqs) words in the image's layout (sequence s at word (offsets[s] >> 5) + s, base i of a word at bit
 * 31 - i).  Only the bits DUST set are set: those of N's are not.  BNS_ERR_STATE while off.  Needs no encoder, table or taxonomy. */
int bns_set_dust(bns_ctx *ctx, uint32_t window, uint32_t level);
int bns_dust_mask(bns_ctx *ctx, const char *bases, const uint64_t *offsets, uint64_t n_seqs, uint32_t *flags);
/* device -> device copy on the context's stream (a caller that keeps text in HBM moves the unconsumed tail in front of the next batch) */
int bns_dev_copy(bns_ctx *ctx, void *dst, const void *src, size_t bytes);
/* ... and between two contexts, src in src_ctx's device memory, dst in dst_ctx's (one device or two: the unconsumed tail of a block that
 * the NEXT device goes on with, when the blocks of one input go to several devices in turn).  Synchronous; waits for no stream of src_ctx.
 * Replaces nothing in the reference (one address space: classifier.h:296-337 keeps its chunk in host memory). */
int bns_dev_copy_peer(bns_ctx *dst_ctx, void *dst, bns_ctx *src_ctx, const void *src, size_t bytes);

/* ---- BGZF members inflated on the device (host ingest) ------------------------------------
 * Replaces, for blocked-gzip input, the reference's one zlib stream (gzFile behind kseq: kseq_declare.h:112-145,
 * klib/kseq.h:177-225 -- ks_getuntil over gzread).  A BGZF file is a sequence of independent gzip members of at most 64 KiB of
 * text; the caller finds them from their 'BC' subfields (no inflating needed) and hands a batch of raw-DEFLATE payloads over:
 * one member per WAVEFRONT, its 64 lanes decoding speculatively at every bit position of a round (csrc/bns_inflate_wave.hpp; 53 GB/s
 * of text at 4 k members per call; BNS_INFLATE_FORM=lane: the round-4 form, one member per lane).  A handle of its own -- stream and staging buffers
 * -- independent of any bns_ctx, so a reader thread inflates while classify calls run; one call at a time per handle.
 *   comp[in_off[i] .. + in_len[i])   member i's DEFLATE payload (between the gzip header and the CRC32/ISIZE trailer)
 *   text[out_off[i] .. + out_len[i]) where its text goes; out_len[i] = the member's ISIZE
 *   crc32[i]                         CRC-32 of the bytes written (compare with the member's trailer)
 *   status[i]                        0, or a BNS_INF_* code (damaged stream, size mismatch): the member's text is then unspecified
 * Host buffers; page-locked ones (bns_inflater_host_alloc) travel at the full link rate.  Returns BNS_OK when the batch ran --
 * per-member failures are reported through status[], not the return value. */
typedef struct bns_inflater bns_inflater;
#define BNS_INF_OK            0
#define BNS_INF_BAD_BLOCK     1
#define BNS_INF_BAD_STORED    2
#define BNS_INF_BAD_LENGTHS   3
#define BNS_INF_BAD_CODE      4
#define BNS_INF_BAD_DISTANCE  5
#define BNS_INF_OUT_OVERFLOW  6
#define BNS_INF_IN_OVERRUN    7
#define BNS_INF_OUT_SHORT     8
int bns_inflater_create(int device, bns_inflater **out);
void bns_inflater_destroy(bns_inflater *h);
const char *bns_inflater_error(const bns_inflater *h);
float bns_inflater_last_kernel_ms(const bns_inflater *h);      /* HIP-event time of the last batch's kernel (< 0: none) */
int bns_inflater_host_alloc(bns_inflater *h, size_t bytes, void **out);
int bns_inflater_host_free(bns_inflater *h, void *p);
int bns_inflate_members(bns_inflater *h, const uint8_t *comp, uint64_t comp_bytes, const uint64_t *in_off, const uint32_t *in_len,
                        const uint64_t *out_off, const uint32_t *out_len, uint64_t n_members, uint8_t *text, uint64_t text_bytes,
                        uint32_t *crc32, uint32_t *status);

/* The same batch with the text LEFT ON THE DEVICE: d_text (device memory of the same GPU, e.g. bns_dev_alloc) receives member i's
 * text at d_text + out_off[i]; only crc32[] and status[] come back.  What bns_classify_text(..., BNS_TEXT_DEVICE) then parses and
 * classifies where it lies: a BGZF file's text never crosses PCIe (compressed bytes up, results down). */
int bns_inflate_members_device(bns_inflater *h, const uint8_t *comp, uint64_t comp_bytes, const uint64_t *in_off, const uint32_t *in_len,
                               const uint64_t *out_off, const uint32_t *out_len, uint64_t n_members, void *d_text, uint64_t text_bytes,
                               uint32_t *crc32, uint32_t *status);

/* ---- ONE plain gzip stream inflated on the device (csrc/bns_gzstream.hip).  Replaces gzread under kseq for a .gz file that is
 * not BGZF (kseq_declare.h:112-145, klib/kseq.h:177-225: one zlib inflate per file).  A DEFLATE stream has no entry points, but a
 * dynamic-Huffman block header is redundant enough to be found: the call's compressed bytes are cut into chunks, a wavefront per chunk
 * finds the first header in it and decodes from there to the next chunk's header -- writing 16-bit symbols, a byte or "byte j of the
 * 32 KiB in front of my entry point" --, one block then walks the chunks in order (each must end exactly where the next begins, else
 * the rest is left for the next call), resolves every chunk's 32 KiB window and the symbols become text, compacted into d_text.
 *   comp[0, comp_bytes)  HOST: a stretch of ONE gzip member's DEFLATE data (< 2 GiB); page-locked memory travels at the link rate
 *   start_bit            bit position in comp of a block header: the member's first block, or where the call before ended
 *   d_window             DEVICE: the 32 KiB of text in front of start_bit (NULL: the member starts there, nothing lies in front)
 *   d_text / text_cap    DEVICE: where the text goes, and its room
 *   d_window_out         DEVICE: receives the 32 KiB of text behind what the call took (the next call's d_window; may be d_window)
 * The call takes whole blocks only.  out->end_bit: behind the last block taken -- a block header (go on from there with more bytes:
 * comp of the next call must hold the stream from bit end_bit & ~7 on), or, with member_end, the first bit behind the member's final
 * block (the trailer follows at the next byte boundary: CRC-32 and ISIZE are the caller's to check, out->crc32 is the CRC-32 of the
 * text_bytes bytes this call wrote; bns_crc32_combine joins the calls of a member).  out->status != BNS_INF_OK: the first chunk
 * made no progress -- BNS_INF_IN_OVERRUN: its first block does not end inside comp (pass more bytes); BNS_INF_OUT_OVERFLOW: it
 * does not fit text_cap or the per-chunk room (BNS_GZ_RATIO_CAP x chunk, default 16 x 64 KiB of symbols); anything else: damaged
 * data.  Returns BNS_OK when the kernels ran. */
typedef struct bns_gz_result {
    uint64_t text_bytes;
    uint64_t end_bit;
    uint32_t member_end;
    uint32_t crc32;
    uint32_t n_chunks;      /* chunks that found a block header (the first one included) */
    uint32_t n_chained;     /* ... whose text this call took */
    uint32_t status;
    uint32_t stop_why;      /* 0 every chunk taken; 1 a chunk did not end at the next header (a false header: decoded again by the next call);
                               2 text room; 3 the member ended; 4 a chunk made no progress */
} bns_gz_result;
int bns_inflate_stream_device(bns_inflater *h, const uint8_t *comp, uint64_t comp_bytes, uint64_t start_bit, const void *d_window, void *d_text,
                              uint64_t text_cap, void *d_window_out, bns_gz_result *out);
/* The device buffers of bns_inflate_stream_device sized NOW for calls of up to comp_bytes (symbols: 2 x BNS_GZ_RATIO_CAP bytes per byte
 * of the stream; a 256 MiB call: ~10 GB): a buffer that grows between two calls is freed and allocated again with the device drained. */
int bns_inflate_stream_reserve(bns_inflater *h, uint64_t comp_bytes);
/* A chunk's room for symbols, per byte of the chunk (2-1024; 0: the default, BNS_GZ_RATIO_CAP or 16).  A call whose first block inflates
 * beyond its chunk's room reports BNS_INF_OUT_OVERFLOW: the caller may ask again with more room and fewer bytes (the buffers are
 * chunks x room: eight times the room on an eighth of the bytes is the same memory) -- text that compresses 100:1 and more. */
int bns_inflate_stream_room(bns_inflater *h, uint32_t symbols_per_byte);
/* A range of host bytes brought up AHEAD, on a stream of its own (two ranges are kept): a later bns_inflate_stream_device call whose
 * comp[0, comp_bytes) lies inside it reads the bytes where they are instead of copying them up first -- the next call's upload under
 * this call's kernels.  The host bytes must not change between the prefetch and the calls that use it; a range is forgotten when the
 * second prefetch after it takes its buffer. */
int bns_inflate_stream_prefetch(bns_inflater *h, const uint8_t *comp, uint64_t comp_bytes);
/* zlib's crc32_combine: the CRC-32 of A followed by B from crc(A), crc(B) and B's length */
uint32_t bns_crc32_combine(uint32_t crc1, uint32_t crc2, uint64_t len2);

#ifdef __cplusplus
}
#endif
#endif /* BONSAI_AMD_H */
