/*
 * pangene_hip.h -- thin C ABI between the host side of the graph-construction path and the code that
 * owns the per-hit data ("backend").  Plain pointers and sizes only; no torch / C++ types.
 *
 * The reference (lh3/pangene v1.1-r231) has no FFI layer: its per-hit work is reached through
 * pg_read_paf()'s tail (read.c:243-260), pg_post_process() (graph.c:7-32) and pg_graph_gen()
 * (graph.c:280-322).  Each entry point below replaces the per-hit loops named in its comment; the
 * S/A-sized logic between them (vertex greedy, branch marking, pruning, formatting) stays on the host
 * (pangene_amd.h).
 *
 * Two implementations of this ABI exist:
 *   pga_*  (libpangene_amd.so)  hand-written HIP kernels for gfx950 -- the product; fails loudly
 *                               without a GPU, has no CPU fallback.
 *   pgo_*  (oracle/liboracle.so) plain-C restatement -- TEST INFRASTRUCTURE ONLY (checker).
 * Both export the same functions (prefix differs) and a vtable (pga_backend()/pgo_backend()).
 *
 * Memory spaces: pointers handed IN are host memory unless stated.  Pointers handed OUT through a
 * `**` argument live in the backend's space (HBM for pga_*, host for pgo_*) and stay valid until the
 * next call of the same function or pga_destroy(); they are what the exchange (all-reduce /
 * all-gather over RCCL) operates on.  Use fetch() to copy them to the host.
 *
 * Canonical order: X = hits sorted by (genome, contig, cs, file index);
 * Y = hits sorted by (genome, contig, cm, X position).  Both are computed once; keys never change.
 */
#ifndef PANGENE_HIP_H
#define PANGENE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* per-hit flag word: same bit positions as the bitfield at pangene.h:70 (rev:1 flt:1 ... weak_br:2) */
#define PGA_F_REV        0x001u
#define PGA_F_FLT        0x002u
#define PGA_F_ISO_SUB    0x004u  /* flt_iso_sub_self */
#define PGA_F_ISO_OV     0x008u  /* flt_iso_ov */
#define PGA_F_CHAIN      0x010u  /* flt_chain */
#define PGA_F_PSEUDO     0x020u
#define PGA_F_VTX        0x040u
#define PGA_F_SHADOW     0x080u
#define PGA_F_REP        0x100u
#define PGA_F_WEAK_SHIFT 9
#define PGA_F_WEAK_MASK  0x600u

/* which field PG_SET_FILTER (pgpriv.h:109-116) tests */
enum { PGA_FLT_PSEUDO = 0, PGA_FLT_VTX0 = 1, PGA_FLT_WEAK2 = 2, PGA_FLT_SHADOW = 3 };

/* status codes: 0 ok; negative = error (never aborts the process) */
enum {
	PGA_OK = 0,
	PGA_ERR_NO_DEVICE = -1,   /* no usable MI355X / HIP runtime error */
	PGA_ERR_RANGE = -2,       /* a coordinate or id does not fit the device layout */
	PGA_ERR_ARG = -3,
	PGA_ERR_NOMEM = -4,
	PGA_ERR_INVARIANT = -5    /* an invariant the reference asserts (e.g. vertex.c:38) was violated */
};

/* One genome of a shard, packed by the host right after its PAF has been parsed (pg_read_paf / pg_read_paf_batch), in FILE
 * order: what read.c:128-236 leaves in pg_genome_t::hit / ::exon (pangene.h:44-46,61-72,79-87), structure-of-arrays.
 * `data` is ONE buffer (pinned host memory when it came from host_alloc(), so the upload is a plain DMA):
 *   10 planes of n_hit int32:  pid, cid, rank, score_ori, score_adj, n_exon, off_exon (into THIS genome's exon list), cs, ce, cm
 *   n_hit bytes rev, padded to a multiple of 4
 *   n_exon pairs of int32 (os, oe), relative to cs, ascending (pangene.h:44-46)
 * The maxima let the backend size its sort keys without looking at the data on the host. */
#define PGA_BLOCK_PLANES 10
typedef struct {
	int32_t n_hit, n_exon, n_ctg;
	int32_t max_cs, max_cm, max_score_adj;   /* over the hits of the genome; 0 when it has none */
	int32_t any_neg_score_adj, any_multi_exon;
	const int32_t *data;
	size_t n_words;                          /* 10 * n_hit + (n_hit + 3) / 4 + 2 * n_exon */
	/* 64-bit contig coordinates (pangene.h:71: int64_t cs, cm, ce) through a 32-bit device layout: VIRTUAL CONTIGS.  A contig whose
	 * coordinates do not fit 31 bits is cut by the packer at hit-free gaps into pieces of < 2^30 bp plus one cluster of overlapping hits; the
	 * block then counts the pieces as contigs (n_ctg, the contig plane) and stores cs / ce / cm relative to the piece's base.  No hit
	 * spans a cut, so every overlap test, sort and filter works on the pieces unchanged; the steps that look ACROSS hits of one contig
	 * -- the walk of pg_gen_arc (graph.c:113-121: same-contig test, dist = cm - vpos, which the reference itself truncates to int32_t,
	 * graph.c:73) and pg_gen_rep_pos / pg_n_local (branch.c:6-46: same contig, 64-bit |cm1 - cm2|) -- put the pieces together again
	 * with these two tables.  vfirst[v] = the first piece of the contig piece v belongs to (the contig's identity; v itself for a contig
	 * that was not cut); vbase[v] = what was subtracted from the coordinates of piece v.  Both NULL: no contig of the genome was cut.
	 * The pieces of a contig are consecutive and in coordinate order (vfirst[v] <= v, vfirst[v] == vfirst[v - 1] or v, vbase not decreasing
	 * inside a contig: PGA_ERR_ARG otherwise), and every hit of piece v + 1 starts AFTER the last base of piece v (the packer's rule:
	 * graph_driver.cpp, virtual_contigs) -- the (contig, cs) and (contig, cm) orders of the pieces are then those of the contig. */
	const int32_t *vfirst;                   /* [n_ctg] or NULL */
	const int64_t *vbase;                    /* [n_ctg] or NULL */
} pga_genome_block_t;

/* One shard = a set of genomes with all their hits (pg_hit_t pangene.h:61-72, pg_exon_t 44-46, pg_genome_t 79-87).
 * Every hit is checked on the device against what its block declares (contig id < n_ctg, 0 <= cs <= ce, cs <= max_cs, cm <= max_cm,
 * score_adj <= max_score_adj or any_neg_score_adj, exon range inside the block's exon list, n_exon > 1 only with any_multi_exon):
 * pga_create answers PGA_ERR_RANGE for a block that breaks its own declaration instead of indexing out of bounds later.
 * Device layout limits (PGA_ERR_RANGE otherwise): coordinates inside a block < 2^31 (contigs beyond that arrive as virtual contigs,
 * see pga_genome_block_t; what remains out of reach is a single cluster of overlapping hits spanning 2^30 bp), < 2^30 hits and < 2^31
 * exons per shard, < 2^20 genes, < 2^24 genomes. */
#define PGA_ABI_VERSION 25u /* bumped whenever a struct of this header or the order of pga_backend_t changes; pga_create refuses another */
typedef struct {
	uint32_t abi_version;        /* = PGA_ABI_VERSION of the header the caller was compiled against (PGA_ERR_ARG otherwise) */
	int32_t n_genome;            /* genomes in this shard (may include genomes with 0 hits) */
	int32_t n_genome_global;     /* G of the whole run (all shards) */
	const int32_t *genome_global;/* [n_genome] global genome index of each local genome */
	int32_t n_prot, n_gene;      /* global table sizes (ids are assigned on the host before upload) */
	int64_t n_hit, n_exon;       /* sums over the blocks */
	const pga_genome_block_t *block; /* [n_genome] */
	const int32_t *prot_gid;     /* [n_prot] */
	const uint8_t *gene_pref;    /* [n_gene] pg_gene_t::preferred */
} pga_shard_t;

typedef struct {
	double  min_ov_ratio;        /* pg_opt_t::min_ov_ratio (overlap.c:136) */
	int32_t check_strand;        /* PG_F_CHECK_STRAND */
	int32_t drop_sgl_exon;       /* PG_F_DROP_SGL_EXON (hit.c:180) -- evaluated on the host, kept for reference */
	int32_t reserved[4];
} pga_params_t;

/* per-hit state, FILE order, host memory (any pointer may be NULL = not wanted) */
typedef struct {
	uint32_t *flags;             /* PGA_F_* */
	int32_t *rank, *score_dom, *pid_dom, *pid_dom0;
	int32_t *pos_x;              /* position of the hit inside its genome in X (cs) order */
	int32_t *pos_y;              /* position of the hit inside its genome in Y (cm) order */
	uint64_t *flt_x_bits;        /* [(n_hit+63)/64] bit (hit_off[g] + pos_x) = flt of that hit: all the W-line writer needs */
} pga_hit_state_t;

/* one partially reduced arc: sums over the LOCAL genomes of the per-genome collapsed values
 * (graph.c:128-145 then the integer part of 153-169); final roundings are done on the host after
 * the cross-shard merge */
typedef struct {
	uint64_t x;                  /* v<<32|w, v = sid<<1|rev */
	int32_t  n_genome, tot_cnt;
	uint64_t sum_dist;           /* sum over genomes of dist_genome * n_genome_local_count */
	int64_t  sum_s1, sum_s2;     /* sum over genomes of per-genome max s1 / s2 */
} pga_arc_part_t;

typedef struct pga_ctx pga_ctx_t;

/* hazard counters: situations in which the reference's unstable sort could make its
 * output depend on tie order.  0 everywhere = canonical order provably gives the reference's result. */
typedef struct {
	int64_t h1_head_tie;         /* index-0 quirk outcome depends on who sits at index 0 */
	int64_t h2_cm_tie;           /* two walkable hits share (contig, cm) */
	int64_t h2_cs_tie;           /* walkable hits sharing (contig, cs) get pg_gen_rep_pos's counter r in tie order (branch.c:14,22-24): counts the
	                              * pg_n_local evaluations (branch.c:31-46) whose |r1 - r2| <= local_count test is not the same for every order of
	                              * the tie group(s) (interval form), and tie groups holding two walkable hits of one gene */
	int64_t h3_dom_tie;          /* dominator arg-max tie / subopt-isoform tie at equal (contig, cs) */
} pga_hazard_t;

#define PGA_HAZARD_CAP 4096

#define PGA_DECLARE(pfx) \
	/* copy a shard (file order) into backend memory; nothing is computed yet */ \
	int  pfx##_create(pga_ctx_t **ctx, const pga_shard_t *sh, const pga_params_t *par); \
	void pfx##_destroy(pga_ctx_t *ctx); \
	/* (re)start a run on the resident shard: per-hit constants (gene id, CDS length pg_cds_len \
	 * overlap.c:45-51, 64-bit score), X and Y orders (pg_hit_sort hit.c:29-64), all state reset to what \
	 * read.c:133-134 leaves after parsing.  May be called again to repeat the run without re-uploading. */ \
	int  pfx##_begin(pga_ctx_t *ctx); \
	/* stage A, read.c:243-260: pg_flag_pseudo, PG_SET_FILTER(pseudo), sort, pg_shadow(cal_dom_sc=1), \
	 * pid_dom0/reset, pg_flt_ov_isoform, pg_flt_chain_shadow, pg_flt_subopt_isoform. \
	 * stats: [n_genome*4] n_pseudo, n_flt_ov_iso, n_flt_chain, n_flt_subopt (host; may be NULL) */ \
	int  pfx##_ingest(pga_ctx_t *ctx, int32_t *stats); \
	/* stage B partials: max_ori[P] = max score_ori over all hits (hit.c:230-238); sums[6P] = \
	 * {sum score_adj, count} of rank-0 non-flt hits (hit.c:196-204) and c0,c1,s0,s1 (hit.c:158-169), \
	 * stored as six planes of P int64 */ \
	int  pfx##_post_partials(pga_ctx_t *ctx, int32_t **max_ori, int64_t **sums); \
	/* cap score_dom (hit.c:239-246, using the reduced max_ori still in backend memory), hit.rep \
	 * (hit.c:219-224), joint pseudo flag for single-exon hits of proteins with prot_pj[pid] (hit.c:170-184) */ \
	int  pfx##_post_apply(pga_ctx_t *ctx, const uint8_t *prot_rep, const uint8_t *prot_pj, int64_t *n_pseudo); \
	/* pg_shadow (overlap.c:101-178) over every genome. stats: [n_genome*2] {#non-flt, #shadowed} or NULL */ \
	int  pfx##_shadow(pga_ctx_t *ctx, int32_t cal_dom_sc, int32_t *stats); \
	/* PG_SET_FILTER (pgpriv.h:109-116) */ \
	int  pfx##_set_filter(pga_ctx_t *ctx, int32_t which); \
	/* pg_gen_vtx per-genome part (vertex.c:28-51): cnt[2Q] = n_dom[Q] then n_sub[Q]; records of \
	 * 1 + ceil(n_genome_global / 64) words: sub_gene<<20 | dom_gene, then the set (bit = global genome index) of this \
	 * shard's genomes in which sub_gene is sub-ordinate to dom_gene and dom_gene is dominant (the only cells the greedy \
	 * vertex.c:60-80 can observe).  A (sub, dom) key may occur in more than one record; their sets are disjoint. */ \
	int  pfx##_vtx_partials(pga_ctx_t *ctx, int32_t **cnt, uint64_t **records, int64_t *n_records); \
	/* pg_graph_flag_vtx (graph.c:61-69); g2s: [n_gene] host.  then_filter != 0: followed at once by PG_SET_FILTER(vtx == 0), \
	 * as everywhere in pg_graph_gen (graph.c:287-288,295,312), in the same pass over the hits */ \
	int  pfx##_flag_vtx(pga_ctx_t *ctx, const int32_t *g2s, int32_t n_seg, int32_t then_filter); \
	/* per-genome part of pg_gen_arc (graph.c:97-146) + local reduce-by-key of its global part. \
	 * seg_cnt[2S] = n_genome[S] then tot_cnt[S] (graph.c:125-126); arcs sorted by x */ \
	int  pfx##_arc_round(pga_ctx_t *ctx, int32_t use_ori, int32_t **seg_cnt, pga_arc_part_t **arcs, int64_t *n_arcs); \
	/* cross-shard reduce-by-key of the locally reduced arc tables after their all-gather: `gathered` (backend memory) \
	 * holds W slots of `slot` entries, count[r] (host) of them valid in slot r, each slot sorted by x.  Sums the \
	 * integer fields of equal x (graph.c:153-169 is a sum, so the order of the shards is irrelevant). */ \
	int  pfx##_arc_merge(pga_ctx_t *ctx, const pga_arc_part_t *gathered, const int64_t *count, int32_t W, int64_t slot, \
	                     pga_arc_part_t **out, int64_t *n_out); \
	/* Declare which arc table in backend memory (the output of arc_round, or of arc_merge when sharded) is the graph's \
	 * arc table of this round.  The backend derives what the following steps read -- per-arc s1 (the double rounding \
	 * of graph.c:171), target gene, the arc range of every oriented vertex -- and keeps it resident, so the arcs only \
	 * travel to the host once, after the last round: branch_pairs(arc_x = NULL), mark_hits(arc_x = NULL) use it. \
	 * deg (host, [2*n_seg]) receives the out-degree of every oriented vertex (pg_flt_high_occ, graph.c:243-250). */ \
	int  pfx##_arc_set_current(pga_ctx_t *ctx, const pga_arc_part_t *arcs, int64_t n_arc, int32_t n_seg, int32_t *deg); \
	/* pg_gen_arc (graph.c:87-177) of a run that is NOT sharded, in one call: the round's table becomes the graph's table at once \
	 * (as after arc_set_current), the host receives seg_cnt[2 * n_seg] (n_genome[S] then tot_cnt[S]), the out-degree of every \
	 * oriented vertex deg[2 * n_seg] after a single wait.  The table itself stays where the backend likes it (arc_table). \
	 * seg_cnt == NULL: nothing waits; the steps that read the table on the backend (rep_pos, branch_pairs, branch_decide) may be \
	 * queued behind it, and arc_round_finish -- to be called before anything that changes the hits (mark_hits, filters) -- \
	 * delivers the two arrays.  It returns 1 when the round has to be repeated (a plain arc_round_local call; whatever was \
	 * queued behind the first one has to be repeated after it as well). */ \
	int  pfx##_arc_round_local(pga_ctx_t *ctx, int32_t use_ori, int32_t n_seg, int32_t *seg_cnt, int32_t *deg); \
	int  pfx##_arc_round_finish(pga_ctx_t *ctx, int32_t n_seg, int32_t *seg_cnt, int32_t *deg); /* seg_cnt = deg = NULL: the status only */ \
	/* the graph's current arc table (of arc_round_local or arc_set_current) as ONE array sorted by x, in backend memory */ \
	int  pfx##_arc_table(pga_ctx_t *ctx, const pga_arc_part_t **arcs, int64_t *n_arc); \
	/* pg_gen_rep_pos (branch.c:6-29) kept in backend memory */ \
	int  pfx##_rep_pos(pga_ctx_t *ctx); \
	/* pg_n_local (branch.c:31-46) for n gene pairs (pairs[2i], pairs[2i+1]) over the local genomes.  The reference only tests the \
	 * result against zero (branch.c:76,86): cnt[i] > 0 iff the pair is local in some local genome; a backend may stop counting \
	 * at the first such genome (the HIP one does), so the exact value is unspecified beyond that */ \
	int  pfx##_n_local(pga_ctx_t *ctx, const int32_t *pairs, int64_t n, int32_t local_dist, int32_t local_count, \
	                   int32_t frag_mode, int32_t **cnt); \
	/* pg_mark_branch_flt_arc (branch.c:48-106), split in two so that the counts can be all-reduced in between. \
	 * branch_pairs: arcs sorted by x with their s1, seg_gid[S] = gene of each segment.  For every oriented vertex \
	 * with >= 2 arcs it lists the gene pairs the reference hands to pg_n_local -- the (best-scoring target, weaker \
	 * target) pairs of branch.c:70-75, then every i<j pair of 83-88 -- and counts each over the local genomes \
	 * (needs rep_pos): cnt[n_pairs] in backend memory.  arc_x = NULL: the table of arc_set_current.  branch_decide (after the all-reduce of cnt): branch.c:76-77 \
	 * and 82-90 -> weak_br per arc (arc_weak: host, n_arc bytes of the table of arc_set_current / branch_pairs(arc_x), or NULL), \
	 * n_dist_loci (host, 2S) and, when asked for (non-NULL), the numbers of arcs marked 1 and 2.  The arcs and their weak_br stay \
	 * resident: mark_hits(NULL, NULL, n_arc) uses them.  n_pairs may be NULL when nobody outside the backend needs the count \
	 * (a run that is not sharded): the backend then does not wait for it either. */ \
	int  pfx##_branch_pairs(pga_ctx_t *ctx, const uint64_t *arc_x, const int32_t *arc_s1, int64_t n_arc, const int32_t *seg_gid, int32_t n_seg, \
	                        double branch_diff, int32_t local_dist, int32_t local_count, int32_t frag_mode, int32_t **cnt, int64_t *n_pairs); \
	int  pfx##_branch_decide(pga_ctx_t *ctx, double branch_diff, double branch_diff_dist, double branch_diff_cut, uint8_t *arc_weak, \
	                         int32_t *n_dist_loci, int64_t *n_flt1, int64_t *n_flt2); \
	/* branch_decide for a run that is not sharded, behind an arc round whose host results have not been collected yet \
	 * (arc_round_local(seg_cnt = NULL)): n_dist_loci stays on the backend, and with do_filter != 0 the three tests of \
	 * pg_flt_high_occ (graph.c:226-258) are made there too -- del[s] = 1 (host, n_seg bytes) when segment s has \
	 * tot_cnt > max_tot_cnt, an oriented vertex with more than max_degree out-arcs, or more than max_dist_loci distant loci \
	 * on a side -- so that the round's counters, degrees and n_dist_loci (12 n_seg words) need not travel; the caller \
	 * then asks arc_round_finish(NULL, NULL) whether the round stands.  Waits.  Returns 2 when the preconditions do not \
	 * hold (the round took the sort path): the caller uses branch_decide + arc_round_finish + its own tests instead. */ \
	int  pfx##_branch_decide_filter(pga_ctx_t *ctx, double branch_diff, double branch_diff_dist, double branch_diff_cut, int32_t do_filter, \
	                                int32_t max_tot_cnt, int32_t max_degree, int32_t max_dist_loci, uint8_t *del); \
	/* pg_mark_branch_flt_hit (branch.c:108-145); arcs sorted by x with their weak_br (0 allowed).  then_filter != 0: followed at \
	 * once by PG_SET_FILTER(weak_br == 2) (graph.c:309), in the same pass over the hits */ \
	int  pfx##_mark_hits(pga_ctx_t *ctx, const uint64_t *arc_x, const uint8_t *arc_weak, int64_t n_arc, int64_t *n_marked, int32_t then_filter); \
	/* Replace the order inside contig segments by the exact order the reference's unstable radix sort \
	 * (ksort.h:52-87) leaves there (computed by the host).  which 0 = cs order (the \
	 * physical array order: index 0 of a genome, first-wins ties), 1 = cm order.  Segment s covers the \
	 * positions [seg_start[s], seg_start[s] + seg_off[s+1]-seg_off[s]) of local genome seg_genome[s]; \
	 * file_idx lists the hits to put there by their FILE index inside the genome. */ \
	int  pfx##_override_order(pga_ctx_t *ctx, int32_t which, int32_t n_seg, const int32_t *seg_genome, const int32_t *seg_start, \
	                          const int64_t *seg_off, const int32_t *file_idx); \
	/* Index-0 channel only (cheap form of override_order): head_file[g] = FILE index of the hit the \
	 * reference has at array index 0 of local genome g (the one pg_shadow never resets, overlap.c:108); \
	 * -1 = the first hit of the canonical order */ \
	int  pfx##_set_head(pga_ctx_t *ctx, const int32_t *head_file); \
	/* copy backend memory to the host / host to backend / backend to backend */ \
	int  pfx##_fetch(pga_ctx_t *ctx, void *dst_host, const void *src_backend, size_t nbytes); \
	int  pfx##_put(pga_ctx_t *ctx, void *dst_backend, const void *src_host, size_t nbytes); \
	int  pfx##_copy(pga_ctx_t *ctx, void *dst_backend, const void *src_backend, size_t nbytes); \
	/* one reusable scratch buffer in backend memory (staging area for padded all-gathers); a second \
	 * call invalidates the first pointer */ \
	int  pfx##_scratch(pga_ctx_t *ctx, size_t nbytes, void **ptr); \
	/* wait until everything issued so far has finished (only needed before handing backend memory to code that does not \
	 * run on the backend's stream; fetch and the calls that return host values synchronise by themselves) */ \
	int  pfx##_sync(pga_ctx_t *ctx); \
	/* fetch without waiting: the bytes are copied to host memory owned by the backend, *host_view points at them and is \
	 * valid from the next synchronising call (fetch, sync, arc_set_current, ...) until the next fetch_later */ \
	int  pfx##_fetch_later(pga_ctx_t *ctx, const void *src_backend, size_t nbytes, const void **host_view); \
	/* pangene.js gfa2matrix (pangene.js:1168-1247) as a reduction over what the W-lines would contain.  ctg_counts: the number \
	 * of hits that survive (flt == 0) on every contig of the shard (genome-major list of contigs, host array of that length): \
	 * a contig prints a W-line iff it has one (format.c:209).  gene_matrix: asm_of_ctg[contig] = column of the contig's \
	 * sample#haplotype (-1: none); mat[n_seg * n_asm] (host) receives, per segment and column, the number of surviving hits of \
	 * the segment's gene on the column's contigs, i.e. the occurrences of the segment in that assembly's walks */ \
	int  pfx##_ctg_counts(pga_ctx_t *ctx, int32_t *cnt); \
	int  pfx##_gene_matrix(pga_ctx_t *ctx, const int32_t *asm_of_ctg, int32_t n_asm, int32_t n_seg, int32_t *mat); \
	/* per-hit state in file order */ \
	int  pfx##_download(pga_ctx_t *ctx, const pga_hit_state_t *out); \
	int  pfx##_hazards(pga_ctx_t *ctx, pga_hazard_t *out); \
	/* where the h2_cm_tie / h2_cs_tie / h3_dom_tie events of the run happened: up to cap contig-segment ids (position of the contig in \
	 * the shard's genome-major list of contigs) in segs, one per event, duplicates possible; *n_total = number of events \
	 * (the backend keeps at most PGA_HAZARD_CAP of them: n_total larger than what was returned = list incomplete) */ \
	int  pfx##_hazard_segs(pga_ctx_t *ctx, int32_t *segs, int32_t cap, int64_t *n_total); \
	/* 1 if `**` pointers are device memory (exchange must use the device collective) */ \
	int  pfx##_is_device(void); \
	/* host memory the backend can upload from without staging (hipHostMalloc for pga_*, malloc for pgo_*); usable before \
	 * any context exists: the PAF reader packs every genome into such a buffer as soon as it has been parsed */ \
	int  pfx##_host_alloc(size_t nbytes, void **ptr); \
	void pfx##_host_free(void *ptr); \
	const char *pfx##_strerror(int code);

PGA_DECLARE(pga)

/* pangene.js `call` (pangene.js:812-862), the walk side of bubble calling: which walks pass through which bubble, and the alleles
 * and genes they carry.  Context-free (no shard): the walks and bubbles come from the host, the results go back to it.
 * In:  walks as one array of oriented segments (vertex = segment * 2 + reverse), walk w = step[walk_off[w] .. walk_off[w+1]);
 *      bubble b runs from vertex bub_vs[b] to bub_ve[b] (bub_vs[b] < 0: no bubble, nothing is recorded for it).
 * Out: rec[n_rec], every (bubble, orientation) passage of every walk: a start vertex at st_off followed in the same walk by the
 *      end vertex at en_off (orientation +: vs .. ve; -: ve^1 .. vs^1), ALL earlier starts for each end (the script's quirk), sorted
 *      by (bubble, walk, en_off, st_off, orientation);
 *      rep[r] = the first record of r's bubble whose oriented path (vs .. ve as vertices) equals r's; cnt[r] = how many records have
 *      rep r (0 when r is not a first record);
 *      gene_*[n_gene]: every (bubble, interior segment) once, with the position of its first appearance (interior steps numbered
 *      in record order, st_off+1 .. en_off-1 inside a record), sorted by (bubble, segment).
 * The output arrays belong to the backend and stay valid until its next call_bubbles. */
typedef struct { int32_t bo, walk, st_off, en_off; } pga_call_rec_t; /* bo = bubble * 2 + (orientation < 0) */
typedef struct {
	const int32_t *step; const int64_t *walk_off; int32_t n_walk; int32_t n_seg;
	const int32_t *bub_vs, *bub_ve; int32_t n_bub;
} pga_call_in_t;
typedef struct {
	int64_t n_rec; const pga_call_rec_t *rec; const int32_t *rep, *cnt;
	int64_t n_gene; const int32_t *gene_bub, *gene_seg; const int64_t *gene_first;
} pga_call_out_t;
int pga_call_bubbles(const pga_call_in_t *in, pga_call_out_t *out);

/* Pangenome accumulation curves (include/pangene_amd.h pg_pan_curves) over a gene x assembly presence matrix.  Context-free, like
 * call_bubbles.  In:  bits[n_gene][(n_asm + 31) / 32], bit (a & 31) of word a >> 5 of row g = gene g present in column a (bits past
 *      n_asm are ignored); order[n_perm][n_asm], each row a permutation of the columns, in the order they are added.
 * Out: count[4][n_perm][n_asm]: for order p and k = 1 .. n_asm at [s][p][k - 1] the genes present in at least one of the first k
 *      columns (s = 0, pan), in all of them (1, core), in column order[p][k - 1] and none before it (2, new), in exactly one of them
 *      (3, unique).  The array belongs to the backend and stays valid until its next pan_curves. */
typedef struct {
	const uint32_t *bits; const int32_t *order;
	int32_t n_gene, n_asm, n_perm;
} pga_curves_in_t;
typedef struct { const int32_t *count; } pga_curves_out_t;
int pga_pan_curves(const pga_curves_in_t *in, pga_curves_out_t *out);

/* Pairwise shared items of assemblies (include/pangene_amd.h pg_pan_shared, pangene dist).  Context-free, like pan_curves.
 * In:  bits[n_asm][(n_item + 31) / 32], assembly-major: bit (m & 31) of word m >> 5 of row a = item m is in assembly a; bits past
 *      n_item are zero (the kernel counts them).
 * Out: shared[n_asm][n_asm] = popcount(B_i & B_j), full and symmetric, the diagonal = |B_a|.  The array belongs to the backend and
 *      stays valid until its next pan_shared.  n_asm <= 65 535 (PGA_ERR_RANGE otherwise). */
typedef struct {
	const uint32_t *bits;
	int32_t n_item, n_asm;
} pga_shared_in_t;
typedef struct { const int32_t *shared; } pga_shared_out_t;
int pga_pan_shared(const pga_shared_in_t *in, pga_shared_out_t *out);

/* Gene associations (include/pangene_amd.h pg_pan_assoc, pangene assoc): the gene pairs whose presence over the assemblies is
 * correlated.  Context-free, like pan_shared, of which it is the transpose: an all-pairs popcount over GENE rows that selects on the
 * device and returns a sparse list instead of the square.  With A = n_asm, a = |B_g|, b = |B_h|, s = |B_g & B_h|, V_g = a (A - a)
 * and D = s A - a b: gene g is eligible when min(a, A - a) >= min_count, and a pair g < h of eligible genes is selected when
 * 10^6 D^2 >= r_permille^2 V_g V_h (decided in integers, 128 bits wide) and the sign of D is asked for (sign 0: both, 1: D >= 0,
 * 2: D < 0).
 * In:  bits[n_gene][(n_asm + 31) / 32], gene-major: bit (a & 31) of word a >> 5 of row g = gene g is in assembly a; bits past n_asm
 *      are zero.  min_count >= 1, 0 <= r_permille <= 1000, max_pair >= 0 (PGA_ERR_ARG otherwise).
 * Out: n_pair selected pairs as pair[n_pair][3] = (g, h, s), g < h, ascending by (g, h), and count[n_gene] = |B_g|.  The arrays
 *      belong to the backend and stay valid until its next pan_assoc.  More than max_pair selected pairs: PGA_ERR_RANGE with n_pair =
 *      the number that passed and pair = NULL.
 * Limits (PGA_ERR_RANGE otherwise): n_asm <= 16 777 215 (both sides of the comparison then stay below 2^112), n_gene <= 16 777 215,
 * and at most 4 194 304 eligible genes (the upper-triangle tiles of the eligible rows are one 1-D grid with an int32 tile number). */
typedef struct {
	const uint32_t *bits;
	int32_t n_gene, n_asm, min_count, r_permille, sign;
	int64_t max_pair;
} pga_assoc_in_t;
typedef struct {
	int64_t n_pair;
	const int32_t *pair;
	const int32_t *count;
} pga_assoc_out_t;
int pga_pan_assoc(const pga_assoc_in_t *in, pga_assoc_out_t *out);

/* Gene-trait association (include/pangene_amd.h pg_pan_trait, pangene trait): the label-permutation test of one binary trait against
 * every gene.  Context-free, like pan_assoc.  Over N = n_col columns (the caller has already dropped the columns where the trait is
 * missing), with y the label row, t = |y|, a = |B_g|, s = |B_g & y|, D = s N - a t: permutation p = 1 .. n_perm of the labels is
 * y_p[r] = y[o_p[r]] with o_p order p of N columns as pan_curves defines it (Fisher-Yates from the last column down,
 * j = next() % (i + 1), splitmix64 started from mix((seed << 32) | p)), made on the device from the one label row; s_p = |B_g & y_p|,
 * D_p = s_p N - a t, and k[g] = #{p : |D_p| >= |D|} for an eligible gene (min(a, N - a) >= min_count), 0 for another.  All integers.
 * In:  bits[n_gene][(n_col + 31) / 32], gene-major as for pan_assoc, and label[(n_col + 31) / 32] in the same layout; bits past n_col
 *      are zero in both.  min_count >= 1, n_perm >= 0 (PGA_ERR_ARG otherwise).  perm_rows: NULL, or -- for tests only -- room for
 *      min(n_perm, pga_trait_batch()) x (n_col + 31) / 32 words that receive the label rows of the first batch of permutations.
 * Out: a[n_gene], s[n_gene], k[n_gene].  The arrays belong to the backend and stay valid until its next pan_trait.
 * The permutations go through in batches of pga_trait_batch() rows, so device memory is bounded by n_gene, n_col and the batch.
 * Limits (PGA_ERR_RANGE otherwise): n_col <= 16 777 215 (every product then stays below 2^48), n_gene <= 16 777 215,
 * n_perm <= 2^31 - 2. */
typedef struct {
	const uint32_t *bits;
	const uint32_t *label;
	int32_t n_gene, n_col, min_count, n_perm;
	uint32_t seed;
	uint32_t *perm_rows;
} pga_trait_in_t;
typedef struct { const int32_t *a, *s, *k; } pga_trait_out_t;
int pga_pan_trait(const pga_trait_in_t *in, pga_trait_out_t *out);
int32_t pga_trait_batch(void); /* permutations per batch: 65 536, or PANGENE_TRAIT_BATCH */

/* The joins of a tree (include/pangene_amd.h pg_pan_join, pangene tree): neighbour-joining (method 0) or UPGMA (method 1) over a
 * fixed-point distance matrix, in integers throughout.  Context-free, like pan_shared.  Slots 0 .. n - 1 start live, d = q, r = the
 * live slots, R[x] = the sum of d[x][y] over live y, n[x] = 1.  A join takes, over live pairs i < j, the smallest
 * (r - 2) d[i][j] - R[i] - R[j] (NJ) or d[i][j] (UPGMA) in int64, ties to the smallest i and then the smallest j; records
 * (i, j, d_ij, R_i, R_j, r) or (i, j, d_ij, n_i, n_j, r); sets d[i][k] = d[k][i] = floor((d[i][k] + d[j][k] - d_ij) / 2) or
 * floor((n_i d[i][k] + n_j d[j][k]) / (n_i + n_j)) for every other live k; n_i += n_j; slot j retires.  NJ stops at r = 3 with the
 * record (x, y, z, d_xy, d_xz, d_yz) of the live x < y < z; UPGMA at r = 1.
 * In:  q[n][n], symmetric, zero diagonal, |q| < 2^29 (the caller's promise; an entry that breaks the last part raises the range flag).
 * Out: rec[n_rec][6], n_rec = n - 2 (NJ) or n - 1 (UPGMA).  The array belongs to the backend and stays valid until its next pan_join.
 * A distance of 2^30 or more in size on the way: PGA_ERR_RANGE (a flag on the device, read once at the end).
 * Limits: 3 <= n (PGA_ERR_ARG otherwise), n <= 65 535 (PGA_ERR_RANGE). */
typedef struct {
	const int32_t *q;
	int32_t n, method;
} pga_join_in_t;
typedef struct { const int64_t *rec; int32_t n_rec; } pga_join_out_t;
int pga_pan_join(const pga_join_in_t *in, pga_join_out_t *out);

/* Bootstrap replicates of a tree (include/pangene_amd.h pg_pan_boot, pangene tree -b; DESIGN.md section 8 "Bootstrap").  Context-free,
 * like pan_join.  Replicate b >= 1 draws n_item items with replacement: x0 = mix64((seed << 32) | b) with mix64 splitmix64's output
 * function, draw t = 0 .. n_item - 1 is m_t = mix64(x0 + (t + 1) * 0x9E3779B97F4A7C15) % n_item; S_b[i][j] = #{t : m_t in B_i & B_j};
 * q_b = the fixed-point distances of S_b as pangene tree defines them (metric 0 = jaccard, 2 = diff with the replicate's own F);
 * rec_b = the joins of q_b as pan_join defines them.  Everything from the bit rows to the records happens on the device.
 * In:  bits[n_asm][(n_item + 31) / 32], assembly-major as for pan_shared; method as for pan_join; replicates first .. first + n_rep - 1
 *      (first >= 1, n_rep >= 0); draws: NULL, or -- for tests only -- room for n_rep x n_item int32 that receive m_t.
 * Out: rec[n_rep][n_rec][6], n_rec = n_asm - 2 (NJ) or n_asm - 1 (UPGMA).  The array belongs to the backend and stays valid until its
 *      next pan_boot.  A range error in any replicate (diff without a fraction bit left, a distance of 2^30 on the way): PGA_ERR_RANGE.
 * One call takes at most pga_boot_batch(n_asm) replicates (PGA_ERR_ARG otherwise): a device-memory budget of 2 GiB over what a
 * replicate keeps for the call (its counts, its distances and the joins' small arrays: 66 replicates at n_asm = 2 000, 2 at
 * 10 000; never more than 1 024), or PANGENE_BOOT_BATCH.  The caller walks its replicates in such chunks.  The function takes n_asm
 * alone, so the draws and the resampled rows (n_item + n_asm x W words a replicate) are outside that budget: the backend makes them
 * for groups of replicates of at most 256 MiB (one replicate at least; PANGENE_BOOT_ROWS_WORDS=n, in words, lowers that for tests),
 * group after group inside the call.  Device memory of a call: at most 2 GiB + the bit rows + 256 MiB, or one replicate's draws and
 * rows in place of the 256 MiB where those are larger.
 * Limits: those of pan_shared and pan_join: 3 <= n_asm (PGA_ERR_ARG otherwise), n_asm <= 65 535 (PGA_ERR_RANGE). */
typedef struct {
	const uint32_t *bits;
	int32_t n_item, n_asm, metric, method;
	uint32_t seed;
	int32_t first, n_rep;
	int32_t *draws;
} pga_boot_in_t;
typedef struct { const int64_t *rec; int32_t n_rec; } pga_boot_out_t;
int pga_pan_boot(const pga_boot_in_t *in, pga_boot_out_t *out);
int32_t pga_boot_batch(int32_t n_asm);

/* Lineage-aware pairwise comparisons (include/pangene_amd.h pg_pan_pairs, pangene trait -L; DESIGN.md section 8 "Lineage-aware trait
 * test"): per gene and label row, the largest set of leaf pairs of a binary tree that contrast in gene and label and whose paths share
 * no vertex, and the most supporting (11-00) and the most opposing (10-01) pairs such a largest set can have.  Context-free, like
 * pan_trait.  The tree comes as a postfix program over a stack of subtrees: op 0 pushes the next leaf, op 1 joins the top two entries.
 * An entry holds N and F_s for the four leaf types s = (gene bit, label); a typed leaf is N = 0, F_s = 0 for its own s and infeasible
 * for the others, a leaf without a label N = 0 and nothing feasible; a join of l and r is F_s = max(F_s[l] + N[r], N[l] + F_s[r]),
 * N = max(N[l] + N[r], F_s[l] + F_t[r] + one pair over the contrasting (s, t)), values ordered by (pairs, pairs of the run's side); the
 * run for the supporting side and the run for the opposing side give out = (pairs, supp, opp) at the last entry left.
 * In:  op[2 n_leaf - 1] (a well-formed program of n_leaf pushes whose stack never holds more than 16 entries; malformed: PGA_ERR_ARG,
 *      deeper: PGA_ERR_RANGE -- a caller that visits the child with the larger stack need first stays within
 *      floor(log2 n_leaf) + 1 <= 16); bits[n_leaf][(n_gene + 31) / 32], assembly-major as for pan_shared, row k = the k-th pushed leaf,
 *      bits past n_gene zero; label[n_row][n_leaf] int8 (1, 0, negative = none) in the same leaf order.
 * Out: out[n_row][n_gene][3] = pairs, supp, opp.  The array belongs to the backend and stays valid until its next pan_pairs.
 * Limits (PGA_ERR_RANGE otherwise): n_leaf <= 65 535 (pairs <= 32 767: the packed values stay below 2^30), n_gene <= 16 777 215. */
typedef struct {
	const uint8_t *op;
	const uint32_t *bits;
	const int8_t *label;
	int32_t n_gene, n_leaf, n_row;
} pga_pairs_in_t;
typedef struct { const int32_t *out; } pga_pairs_out_t;
int pga_pan_pairs(const pga_pairs_in_t *in, pga_pairs_out_t *out);

/* Quantitative traits (include/pangene_amd.h pg_pan_qtrait, pangene qtrait; DESIGN.md section 8 "Quantitative traits"): the rank-sum
 * permutation test of one quantitative trait against every gene.  Context-free, like pan_trait.  Over N = n_col columns (the caller has
 * already dropped the columns without a value) with c2 the centred doubled midranks of the values (c2 = r2 - (N + 1), sum c2 = 0,
 * |c2| <= N - 1), a = |B_g| and D = the sum of c2 over the columns of B_g: permutation p = 1 .. n_perm is c2_p[r] = c2[o_p[r]] with o_p
 * order p of N columns exactly as pan_trait and pan_curves define it (the same swap sequence run over the value row), D_p = the sum of
 * c2_p over B_g, and k[g] = #{p : |D_p| >= |D|} for an eligible gene (min(a, N - a) >= min_count), 0 for another.  All integers.
 * In:  bits[n_gene][(n_col + 31) / 32], gene-major as for pan_trait, bits past n_col zero; c2[n_col] int16.  min_count >= 1,
 *      n_perm >= 0 (PGA_ERR_ARG otherwise).  perm_rows and d_rows: NULL, or -- for tests only -- room for
 *      min(n_perm, pga_qtrait_batch()) x n_col int16 that receive the permuted rows of the first batch (put together again from the two
 *      digit planes the count kernel reads), and for min(n_perm, pga_qtrait_batch()) x n_gene int32 that receive that batch's D_p.
 * Out: a[n_gene], d[n_gene], k[n_gene].  The arrays belong to the backend and stay valid until its next pan_qtrait.
 * The permutations go through in batches of pga_qtrait_batch() rows, so device memory is bounded by n_gene, n_col and the batch.
 * Limits (PGA_ERR_RANGE otherwise, before anything is launched): n_col <= 32 000 (c2 = 256 hi + lo with both digits signed bytes, and
 * |D| <= N (N - 1) / 2 < 2^30: every sum fits int32), n_gene <= 16 777 215, n_perm <= 2^31 - 2. */
typedef struct {
	const uint32_t *bits;
	const int16_t *c2;
	int32_t n_gene, n_col, min_count, n_perm;
	uint32_t seed;
	int16_t *perm_rows;
	int32_t *d_rows;
} pga_qtrait_in_t;
typedef struct { const int32_t *a, *d, *k; } pga_qtrait_out_t;
int pga_pan_qtrait(const pga_qtrait_in_t *in, pga_qtrait_out_t *out);
int32_t pga_qtrait_batch(void); /* permutations per batch: 16 384, or PANGENE_QTRAIT_BATCH */

/* k-medoids clusters (include/pangene_amd.h pg_pan_medoids, pangene cluster; DESIGN.md section 8 "Clusters"): PAM over a fixed-point
 * distance matrix, in integers throughout.  Context-free, like pan_join.  TD(M) = the sum over o of the smallest q[o][m], m in M.
 * BUILD: M empty, D[o] = 2^29; k times, over x not in M, the largest gain(x) = sum over o of max(0, D[o] - q[x][o]), ties to the smallest
 * x; M += x, D[o] = min(D[o], q[x][o]); record (x, -1, gain).  SWAP, at most max_iter times: over x not in M and m in M the smallest
 * delta(x, m) = TD(M - m + x) - TD(M), ties to the smallest x and then the smallest m (assembly indices); delta >= 0: converged, stop;
 * otherwise M = M - m + x and the record is (x, m, delta).  Result: the medoids ascending, cluster c = the c-th of them; a medoid labels
 * itself, any other o takes the medoid with the smallest (q[o][m], m); dist[o] = q[o][medoid of o]; size[c]; td = TD(M);
 * sums[o][c] = the sum of q[o][p] over the p of cluster c.
 * In:  q[n][n], symmetric, zero diagonal, 0 <= q < 2^29 (the caller's promise: pg_pan_medoids checks it before it calls).
 * Out: medoid[k], label[n], dist[n], size[k], sums[n][k], rec[n_rec][3] with n_rec = k + n_swap, td, converged (1: an iteration found no
 *      negative delta; 0: max_iter iterations all swapped).  The arrays belong to the backend and stay valid until its next pan_medoids.
 * The swap iterations are queued in chunks of 8 (PANGENE_MEDOIDS_BATCH, for tests) with one read of the status a chunk;
 * PANGENE_MEDOIDS_ROWS (tests) fixes the rows a workgroup of the swap kernel walks.
 * Limits: n >= 3, 2 <= k <= n - 1, max_iter >= 0 (PGA_ERR_ARG otherwise); n <= 65 535, k <= 1 024 (PGA_ERR_RANGE, before anything is
 * launched).  Device memory: the matrix, n x k int64 twice over, and a few arrays of n. */
typedef struct {
	const int32_t *q;
	int32_t n, k, max_iter;
} pga_medoids_in_t;
typedef struct {
	const int32_t *medoid, *label, *dist, *size;
	const int64_t *sums, *rec;
	int64_t td;
	int32_t n_rec, n_swap, converged;
} pga_medoids_out_t;
int pga_pan_medoids(const pga_medoids_in_t *in, pga_medoids_out_t *out);

/* PERMANOVA (include/pangene_amd.h pg_pan_permanova, pangene permanova; DESIGN.md section 8 "PERMANOVA"): do the two groups of one binary
 * label row differ in a fixed-point distance matrix as a whole.  Context-free, like pan_trait.  Over n columns (the caller has already
 * dropped the columns without a label) with e = q >> shift and w[i][j] = e[i][j]^2 (int64, zero diagonal): r[i] = the sum of w[i][.],
 * T = the sum of r, A(y) = the sum of y_i y_j w[i][j] over ordered pairs, B(y) = the sum of y_i r[i], G(y) = n A(y) - 2 n1 B(y) in
 * 128 bits.  Permutation p = 1 .. n_perm is y_p[r] = y[o_p[r]], o_p = order p of n columns exactly as pan_trait defines it, and
 * k = #{p : G(y_p) <= G(y)}.  All integers.
 * In:  q[n][n], symmetric, zero diagonal, 0 <= q <= q_max, and shift with (q_max >> shift)^2 n (n - 1) < 2^62, so that T, A and B stay
 *      below 2^62 (the caller's promise: pg_pan_permanova checks the matrix and derives shift before it calls); label[(n + 31) / 32], bit c =
 *      y_c, bits past n zero; n1 = the set bits.  a_rows, b_rows, perm_rows: NULL, or -- for tests only -- room for
 *      min(n_perm, pga_permanova_batch()) int64 each that receive A and B of the first batch's permutations, and for as many rows of
 *      (n + 31) / 32 words that receive its label rows.
 * Out: t, a and b of the observed row, and k.
 * The permutations go through in batches of pga_permanova_batch() rows; device memory is the matrix, its D <= 8 signed-byte digit
 * planes of (n rounded up to 128)^2 bytes and the batch's rows.
 * Limits: n >= 1, n_perm >= 0, 0 <= shift < 31, 0 <= n1 <= n (PGA_ERR_ARG otherwise); n <= 16 384, n_perm <= 2^31 - 2 (PGA_ERR_RANGE,
 * before anything is launched). */
typedef struct {
	const int32_t *q;
	const uint32_t *label;
	int32_t n, shift, q_max, n1, n_perm;
	uint32_t seed;
	int64_t *a_rows, *b_rows;
	uint32_t *perm_rows;
} pga_permanova_in_t;
typedef struct { int64_t t, a, b, k; } pga_permanova_out_t;
int pga_pan_permanova(const pga_permanova_in_t *in, pga_permanova_out_t *out);
int32_t pga_permanova_batch(void); /* permutations per batch: 16 384, or PANGENE_PERMA_BATCH */

/* Mantel test (include/pangene_amd.h pg_pan_mantel, pangene mantel; DESIGN.md section 8 "Mantel test"): do two distance matrices of the
 * same n assemblies agree.  Context-free, like pan_permanova.  An order o of the assemblies gives Z(o) = the sum over ordered pairs
 * i != j of a[i][j] b[o[i]][o[j]]; Z of the identity is the observed one, permutation p = 1 .. n_perm uses o_p = order p of n columns
 * exactly as pan_trait defines it, n_ge = #{p : Z_p >= Z}, n_le = #{p : Z_p <= Z} (ties count in both).  All integers.
 * In:  a[n][n] and b[n][n], already shifted: symmetric, zero diagonal, 0 <= a <= max_a, 0 <= b <= max_b and max_a max_b n (n - 1) < 2^62,
 *      so that every Z stays below 2^62 (the caller's promise: pg_pan_mantel checks the matrices and derives the shifts before it calls;
 *      the product is checked here before anything is launched, PGA_ERR_ARG).  z_rows, ord_rows: NULL, or -- for tests only -- room for
 *      min(n_perm, pga_mantel_batch()) int64 that receive Z of the first batch's permutations, and for as many rows of n uint16 that
 *      receive its orders.
 * Out: z of the identity order, n_ge and n_le.
 * The permutations go through in batches of pga_mantel_batch() orders; device memory is the two matrices and the batch's orders.
 * Limits: n >= 1, n_perm >= 0, max_a >= 0, max_b >= 0 (PGA_ERR_ARG otherwise); n <= 16 384, n_perm <= 2^31 - 2 (PGA_ERR_RANGE, before
 * anything is launched). */
typedef struct {
	const int32_t *a, *b;
	int32_t n, max_a, max_b, n_perm;
	uint32_t seed;
	int64_t *z_rows;
	uint16_t *ord_rows;
} pga_mantel_in_t;
typedef struct { int64_t z, n_ge, n_le; } pga_mantel_out_t;
int pga_pan_mantel(const pga_mantel_in_t *in, pga_mantel_out_t *out);
int32_t pga_mantel_batch(void); /* permutations per batch: 4 096, or PANGENE_MANTEL_BATCH */

/* Gene gain and loss on a tree (include/pangene_amd.h pg_pan_gainloss, pangene gainloss; DESIGN.md section 8 "Gain and loss"): Wagner
 * parsimony per item, a gain (parent absent, child present) costing `gain` and a loss `loss`.  Context-free, like pan_pairs, and over the
 * same postfix program: op 0 pushes the next leaf, op 1 joins the top two entries.  Every op makes one node, so a node is named by its op.
 * Up: an entry is (C0, C1); a leaf with bit b has C[b] = 0, C[1 - b] = gain + loss; a join has C[s] = the sum over its two children c of
 * min(C_c[s], C_c[1 - s] + w(s)), w(0) = gain, w(1) = loss.  Down: the root is present iff C1 < C0; a child of a parent in state s
 * switches iff C_c[1 - s] + w(s) < C_c[s] (mode 0, late) or <= (mode 1, early).
 * In:  op[2 n_leaf - 1] as for pan_pairs (malformed: PGA_ERR_ARG, a stack need above 16: PGA_ERR_RANGE); par[2 n_leaf - 1] = the op of
 *      the join that takes the node of each op, -1 for the last op, the root (anything else: PGA_ERR_ARG); bits[n_leaf][(n_gene + 31) / 32]
 *      as for pan_pairs, row k = the k-th pushed leaf; mode 0 or 1 (PGA_ERR_ARG otherwise).  st_rows: NULL, or -- for tests only -- room
 *      for the first chunk's state rows, uint64 [2 n_leaf - 1][ceil(min(n_gene, pga_gainloss_chunk(n_leaf)) / 64)]: bit i & 63 of word
 *      i >> 6 of row k = item i is present at the node of op k; bits past n_gene are zero.
 * Out: gene[n_gene][4] = cost, gains, losses, root state; node[2 n_leaf - 1][3] = in op order the items present at the node and the
 *      gains and losses on the branch above it (0 and 0 for the root).  The arrays belong to the backend and stay valid until its next
 *      pan_gainloss.  n_leaf = 0 or n_gene = 0: zeros, nothing is launched.
 * The items go through in chunks of pga_gainloss_chunk(n_leaf): PANGENE_GAINLOSS_CHUNK rounded up to a multiple of 1 024, or the largest
 * multiple of 1 024 items whose three bit rows per node fit 1 GiB, never less than 1 024.
 * Limits (PGA_ERR_RANGE otherwise, before anything is launched): n_leaf <= 65 535, n_gene <= 16 777 215, 1 <= gain, loss <= 255 (every
 * cost then stays below 2^25). */
typedef struct {
	const uint8_t *op;
	const uint32_t *bits;
	const int32_t *par;
	int32_t n_gene, n_leaf, gain, loss, mode;
	uint64_t *st_rows;
} pga_gainloss_in_t;
typedef struct { const int32_t *gene; const int64_t *node; } pga_gainloss_out_t;
int pga_pan_gainloss(const pga_gainloss_in_t *in, pga_gainloss_out_t *out);
int32_t pga_gainloss_chunk(int32_t n_leaf);

/* Co-evolution (include/pangene_amd.h pg_pan_coevo, pangene coevo; DESIGN.md section 8 "Co-evolution"): the item pairs whose gains and
 * losses fall on the same branches of a tree.  Context-free.  The reconstruction is pan_gainloss's, over the same program, rows and par,
 * with the same checks and limits.  Every op but the last (the root) has one branch above its node: B = 2 n_leaf - 2 branches, named by
 * their op.  Item i has the gain set G_i (node present, parent absent), the loss set L_i (the reverse) and e_i = |G_i| + |L_i| events; it is
 * eligible when e_i >= min_events.  For two eligible items i < j: same = |G_i & G_j| + |L_i & L_j|, opp = |G_i & L_j| + |L_i & G_j|,
 * d = same - opp; the pair is selected when 10^6 d^2 >= r_permille^2 e_i e_j (plain 64-bit: both sides are below 2^54) and sign 0 (both),
 * sign 1 and d >= 0, or sign 2 and d < 0.
 * In:  as for pan_gainloss; min_events >= 1, r_permille in [0, 1000], sign 0, 1 or 2, max_pair >= 0 (PGA_ERR_ARG otherwise).  ev_rows: NULL,
 *      or -- for tests only -- room for ev_cap event rows, uint32 [ev_cap][2][ceil(B / 32)]: row e belongs to the e-th eligible item, plane 0
 *      holds its gains and plane 1 its losses, bit k & 31 of word k >> 5 = the branch above the node of op k; the first min(E, ev_cap) rows
 *      are filled.
 * Out: events[n_gene] = e_i; n_pair = the pairs selected; pair[n_pair][4] = i, j, same, opp in ascending (i, j).  The arrays belong to the
 *      backend and stay valid until its next pan_coevo.  More than max_pair pairs: PGA_ERR_RANGE with n_pair set and pair NULL.
 *      n_leaf < 2 or n_gene = 0: zeros, nothing is launched.
 * The items go through the reconstruction in chunks of pga_coevo_chunk(n_leaf): PANGENE_COEVO_CHUNK rounded up to a multiple of 1 024, or
 * pga_gainloss_chunk(n_leaf).  PANGENE_COEVO_CAP=n sets the number of records the first run of the pairs kernel has room for.
 * Limits (PGA_ERR_RANGE otherwise): those of pan_gainloss, and at most 4 194 304 eligible items. */
typedef struct {
	const uint8_t *op;
	const uint32_t *bits;
	const int32_t *par;
	int32_t n_gene, n_leaf, gain, loss, mode;
	int32_t min_events, r_permille, sign;
	int64_t max_pair;
	uint32_t *ev_rows;
	int64_t ev_cap;
} pga_coevo_in_t;
typedef struct { const int32_t *events; int64_t n_pair; const int32_t *pair; } pga_coevo_out_t;
int pga_pan_coevo(const pga_coevo_in_t *in, pga_coevo_out_t *out);
int32_t pga_coevo_chunk(int32_t n_leaf);

/* Phylogenetic signal (include/pangene_amd.h pg_pan_phylosig, pangene phylosig; DESIGN.md section 8 "Phylogenetic signal"): the
 * permutation tail of the parsimony cost.  Context-free.  The tree is pan_gainloss's postfix program; the null distribution of an item
 * depends only on its number of carriers, so the replicates are classes x permutations.  Replicate (n, p), p = 1 .. n_perm: with o_p the
 * order pgx::fisher_yates_order(n_leaf, seed, p) gives, assembly x is present iff o_p[x] < n; cost(n, p) = min(C0, C1) at the root of
 * pan_gainloss's up pass over that tip set.
 * In:  op[2 n_leaf - 1], checked as pan_gainloss checks it (malformed: PGA_ERR_ARG, a stack need above 16: PGA_ERR_RANGE); leaf[n_leaf]
 *      = the assembly of the k-th push, a permutation of 0 .. n_leaf - 1 (PGA_ERR_ARG otherwise); cls[n_cls] strictly ascending, each in
 *      1 .. n_leaf - 1 (PGA_ERR_ARG otherwise); item_cls[n_item] an index into cls (PGA_ERR_ARG otherwise); item_cost[n_item] the
 *      observed cost.  cost_rows, rank_rows: NULL, or -- for tests only -- room for the first batch's costs, int32 [n_cls][nb], and
 *      orders, uint16 [n_leaf][nbs]: rank_rows[x * nbs + q] = o_(1 + q)[x], nb = min(n_perm, pga_phylosig_batch(n_cls)), nbs = nb rounded
 *      up to a multiple of 64; the columns past nb hold an order nobody reads.
 * Out: n_le[n_item] = #{p : cost(cls[item_cls[i]], p) <= item_cost[i]}, n_ge[n_item] the same with >=, sum[n_cls] = the sum over p of
 *      cost(cls[c], p).  The arrays are page-locked, belong to the backend and stay valid until its next pan_phylosig.  n_cls, n_item or
 *      n_perm = 0: zeros, nothing is launched.
 * The permutations go through in batches of pga_phylosig_batch(n_cls): PANGENE_PHYLOSIG_BATCH rounded up to a multiple of 64, or the
 * largest multiple of 64 up to 4 096 for which n_cls x batch x 4 bytes stay within 256 MiB, never less than 64.
 * Limits (PGA_ERR_RANGE otherwise, before anything is launched): n_leaf <= 65 535, a stack need <= 16, 1 <= gain, loss <= 255,
 * n_perm <= 2^31 - 2, n_item <= 16 777 215. */
typedef struct {
	const uint8_t *op;
	const int32_t *leaf;
	int32_t n_leaf, gain, loss;
	int32_t n_cls; const int32_t *cls;
	int32_t n_item; const int32_t *item_cls;
	const int32_t *item_cost;
	int32_t n_perm; uint32_t seed;
	int32_t *cost_rows;
	uint16_t *rank_rows;
} pga_phylosig_in_t;
typedef struct { const int32_t *n_le, *n_ge; const int64_t *sum; } pga_phylosig_out_t;
int pga_pan_phylosig(const pga_phylosig_in_t *in, pga_phylosig_out_t *out);
int32_t pga_phylosig_batch(int32_t n_cls);

/* Principal coordinates (include/pangene_amd.h pg_pan_pcoa, pangene pcoa; DESIGN.md section 8 "Principal coordinates"): the n_axis
 * algebraically largest eigenpairs of B = J A J, A = -1/2 d o d, d = q 2^-fbits, J = I - 11'/n, by Lanczos with full
 * reorthogonalisation in the centred subspace.  Context-free.  B is never formed: for x orthogonal to 1, B x = A x - mean(A x) 1, and
 * A x comes from q itself, -1/2 d^2 formed in fp64 on the fly.  The first floating-point entry: every sum has a fixed reduction tree,
 * there is no floating-point atomic, and the same call on the same build returns the same bits.
 * In:  q[n][n], symmetric, zero diagonal, 0 <= q < 2^29 (the caller's promise: pg_pan_pcoa checks it); seed of the counter-based start
 *      vectors; max_step: the vectors the iteration may use in all, 1 .. 256 (<= 0: 256).  x_test, y_test, n_test: NULL, NULL, 0, or --
 *      for tests only -- n_test <= 8 columns x_test[n][n_test] (row-major) and room for y_test[n][n_test], which receives
 *      A x - the column means (= B x for columns orthogonal to 1) from the product kernel before the iteration starts.
 * Out: n_axis = min(asked, n - 1, the Ritz values there are) pairs in descending order of the eigenvalue: eig[n_axis], resid[n_axis] (the
 *      residual norm |beta s| of each pair), vec[n][n_axis] (row-major, unit columns orthogonal to 1, no sign convention); n_step (the
 *      vectors used), n_restart (the restarts after an invariant subspace was locked) and converged (every returned pair has a residual
 *      <= 1e-10 times the largest eigenvalue).  The arrays are page-locked, belong to the backend and stay valid until its next pan_pcoa.
 *      Running into max_step is not an error: converged is 0 and the residuals say how far the pairs are.
 * Limits: n >= 1, fbits in [0, 30] (PGA_ERR_ARG otherwise); n <= 16 384 and 1 <= n_axis <= 16 (PGA_ERR_RANGE, before anything is
 * launched); an n_axis above n - 1 is n - 1.  n_test in [0, 8] (PGA_ERR_ARG otherwise). */
typedef struct {
	const int32_t *q;
	int32_t n, fbits, n_axis;
	uint32_t seed;
	int32_t max_step;
	const double *x_test;
	double *y_test;
	int32_t n_test;
} pga_pcoa_in_t;
typedef struct { const double *eig, *resid, *vec; int32_t n_axis, n_step, n_restart, converged; } pga_pcoa_out_t;
int pga_pan_pcoa(const pga_pcoa_in_t *in, pga_pcoa_out_t *out);

/* Structure-adjusted association (include/pangene_amd.h pg_pan_glm, pangene glm; DESIGN.md section 8 "Structure-adjusted association"):
 * the score statistics of every gene against every trait whose null model the host has fitted.  Context-free.  Floating point, fp64
 * throughout: S = X . cols on the fp64 matrix cores (v_mfma_f64_16x16x4_f64), no floating-point atomic, partial sums of fixed segments
 * added in a fixed order; the same call on the same build returns the same bits.
 * In:  bits[n_gene][W], gene-major, W = ceil(n_asm / 32), the bits past n_asm zero (the caller's promise).  cols[n_trait][n_asm][16]:
 *      per trait and assembly 16 doubles (128 bytes) -- column 0 valid (1.0 or 0.0), 1 r, 2 w, 3 .. 2 + n_cov w z_j, the rest zero, the
 *      whole row zero for an assembly without a value: that is how a missing value is handled, the bit rows are never compacted.
 *      chol[n_trait][(n_cov + 1)^2]: the Cholesky factor L of Z'WZ, row-major, lower triangle.  sums_test: NULL, or -- for tests only --
 *      room for [n_trait][n_gene][16] doubles, which receive the raw sums S.
 * Out: a[n_trait][n_gene] = S_0 (the carriers among the assemblies with a value, an exact integer), u = S_1, sw = S_2 and
 *      v = sw - |L^-1 (S_2 .. S_{2 + n_cov})|^2 by forward substitution in ascending order.  The arrays are page-locked, belong to the
 *      backend and stay valid until its next pan_glm.
 * Limits: counts >= 0 (PGA_ERR_ARG otherwise); n_asm <= 16 384, n_cov <= 13, n_gene < 2^24, n_trait <= 4 096 (PGA_ERR_RANGE, before
 * anything is launched). */
typedef struct {
	const uint32_t *bits;
	const double *cols, *chol;
	int32_t n_gene, n_asm, n_trait, n_cov;
	double *sums_test;
} pga_glm_in_t;
typedef struct { const int32_t *a; const double *u, *v, *sw; } pga_glm_out_t;
int pga_pan_glm(const pga_glm_in_t *in, pga_glm_out_t *out);

/* Gain and loss rates (include/pangene_amd.h pg_pan_rates, pangene rates; DESIGN.md section 8 "Gain and loss rates"): the likelihood of
 * every item under a two-state Markov model on the tree, for a batch of parameter sets, and for set 0 the posterior gains, losses and
 * presence.  Context-free, fp64 throughout, over pan_gainloss's postfix program.  The device sees tables only: the host has turned rates
 * and branch lengths into transition probabilities, and no kernel takes an exponential, a logarithm or divides by a rate.
 * Up: a leaf with bit b has in = (1 - b, b); a join has in_v(a) = the product over its two children c of P^c_a0 in_c(0) + P^c_a1 in_c(1);
 * L = pi_0 in_root(0) + pi_1 in_root(1).  After every join both values are divided by 2^e, e the binary exponent (frexp) of the larger
 * one, which is exact, and the exponents add up: L = lik_m 2^lik_e never leaves the range of the pair.
 * Down (post = 1, set 0): out_root = pi; for a child c of v with sibling d, O(a) = out_v(a) (P^d_a0 in_d(0) + P^d_a1 in_d(1)),
 * J(a, b) = O(a) P^c_ab in_c(b), out_c(b) = O(0) P^c_0b + O(1) P^c_1b, Z = the sum of J; present_c = (J01 + J11) / Z, gain_c = J01 / Z,
 * loss_c = J10 / Z (all 0 when Z = 0); at the root present = pi_1 in(1) / L.
 * In:  op, par and bits[n_leaf][(n_gene + 31) / 32] exactly as pan_gainloss takes and checks them.  n_set in 1 .. 64.
 *      tab[n_set][2 n_leaf - 1][4] = P00 P01 P10 P11 of the branch above the node of op k (the root's row is not read), pi[n_set][2]; an
 *      entry that is not finite or is negative: PGA_ERR_ARG.  post 0 or 1.  n_sum in [0, n_gene]: the node totals add the items
 *      [0, n_sum), so that a caller can append a pseudo-item and keep it out of them.  post_rows: NULL, or -- for tests only, with
 *      post = 1 -- room for the first chunk's posterior presence, double [2 n_leaf - 1][min(n_gene, pga_rates_chunk(n_leaf))].
 * Out: lik_m[n_set][n_gene] in [0.5, 1) or 0 and lik_e[n_set][n_gene]; with post, for set 0, gene[n_gene][3] = the sums over the
 *      branches of gain and loss, and the root's present; node[2 n_leaf - 1][3] = in op order the sums over the items of present, gain
 *      and loss (0 and 0 for the root); without post both are NULL.  The arrays are page-locked, belong to the backend and stay valid
 *      until its next pan_rates.  n_leaf = 0 or n_gene = 0: nothing is launched.
 * With post the items go through in chunks of pga_rates_chunk(n_leaf): PANGENE_RATES_CHUNK rounded up to a multiple of 256, or the
 * largest multiple of 256 whose rows (16 bytes per item and node) fit 1 GiB, never less than 256.  No floating-point atomic and fixed
 * reduction orders: the same call on the same build returns the same bits.  PANGENE_RATES_TIMING=1: a line with the kernels' device
 * times on stderr.
 * Limits (PGA_ERR_RANGE otherwise, before anything is launched): n_leaf <= 65 535, n_gene <= 16 777 215, a stack need <= 16,
 * n_set <= 64. */
typedef struct {
	const uint8_t *op;
	const uint32_t *bits;
	const int32_t *par;
	int32_t n_gene, n_leaf, n_set;
	const double *tab, *pi;
	int32_t post, n_sum;
	double *post_rows;
} pga_rates_in_t;
typedef struct { const double *lik_m; const int32_t *lik_e; const double *gene, *node; } pga_rates_out_t;
int pga_pan_rates(const pga_rates_in_t *in, pga_rates_out_t *out);
int32_t pga_rates_chunk(int32_t n_leaf);

/* the same ABI as a table, so the host driver is written once */
struct pga_branch_par_s; struct pga_loop_xchg_s;
typedef struct {
	const char *name;
	int  (*create)(pga_ctx_t **, const pga_shard_t *, const pga_params_t *);
	void (*destroy)(pga_ctx_t *);
	int  (*begin)(pga_ctx_t *);
	int  (*ingest)(pga_ctx_t *, int32_t *);
	int  (*post_partials)(pga_ctx_t *, int32_t **, int64_t **);
	int  (*post_apply)(pga_ctx_t *, const uint8_t *, const uint8_t *, int64_t *);
	int  (*shadow)(pga_ctx_t *, int32_t, int32_t *);
	int  (*set_filter)(pga_ctx_t *, int32_t);
	int  (*vtx_partials)(pga_ctx_t *, int32_t **, uint64_t **, int64_t *);
	int  (*flag_vtx)(pga_ctx_t *, const int32_t *, int32_t, int32_t);
	int  (*arc_round)(pga_ctx_t *, int32_t, int32_t **, pga_arc_part_t **, int64_t *);
	int  (*arc_merge)(pga_ctx_t *, const pga_arc_part_t *, const int64_t *, int32_t, int64_t, pga_arc_part_t **, int64_t *);
	int  (*arc_set_current)(pga_ctx_t *, const pga_arc_part_t *, int64_t, int32_t, int32_t *);
	int  (*rep_pos)(pga_ctx_t *);
	int  (*n_local)(pga_ctx_t *, const int32_t *, int64_t, int32_t, int32_t, int32_t, int32_t **);
	int  (*branch_pairs)(pga_ctx_t *, const uint64_t *, const int32_t *, int64_t, const int32_t *, int32_t, double, int32_t, int32_t, int32_t, int32_t **, int64_t *);
	int  (*branch_decide)(pga_ctx_t *, double, double, double, uint8_t *, int32_t *, int64_t *, int64_t *);
	int  (*mark_hits)(pga_ctx_t *, const uint64_t *, const uint8_t *, int64_t, int64_t *, int32_t);
	int  (*override_order)(pga_ctx_t *, int32_t, int32_t, const int32_t *, const int32_t *, const int64_t *, const int32_t *);
	int  (*set_head)(pga_ctx_t *, const int32_t *);
	int  (*fetch)(pga_ctx_t *, void *, const void *, size_t);
	int  (*put)(pga_ctx_t *, void *, const void *, size_t);
	int  (*copy)(pga_ctx_t *, void *, const void *, size_t);
	int  (*scratch)(pga_ctx_t *, size_t, void **);
	int  (*download)(pga_ctx_t *, const pga_hit_state_t *);
	int  (*hazards)(pga_ctx_t *, pga_hazard_t *);
	int  (*is_device)(void);
	const char *(*strerror)(int);
	int  (*timing_reset)(pga_ctx_t *);  /* may be NULL */
	int  (*timing_get)(pga_ctx_t *, int32_t, double *, int64_t *, int64_t *);
	int  (*sync)(pga_ctx_t *);
	int  (*fetch_later)(pga_ctx_t *, const void *, size_t, const void **);
	int  (*hazard_segs)(pga_ctx_t *, int32_t *, int32_t, int64_t *);
	int  (*host_alloc)(size_t, void **);
	void (*host_free)(void *);
	int  (*arc_round_local)(pga_ctx_t *, int32_t, int32_t, int32_t *, int32_t *);
	int  (*ctg_counts)(pga_ctx_t *, int32_t *);
	int  (*gene_matrix)(pga_ctx_t *, const int32_t *, int32_t, int32_t, int32_t *);
	int  (*arc_table)(pga_ctx_t *, const pga_arc_part_t **, int64_t *);
	int  (*arc_round_finish)(pga_ctx_t *, int32_t, int32_t *, int32_t *);
	int  (*branch_decide_filter)(pga_ctx_t *, double, double, double, int32_t, int32_t, int32_t, int32_t, uint8_t *); /* may be NULL */
	int  (*branch_loop)(pga_ctx_t *, int32_t, const struct pga_branch_par_s *, const int32_t *, const int32_t *, const int32_t *, uint8_t *, const struct pga_loop_xchg_s *, int32_t *, int32_t *); /* may be NULL */
	void (*host_trim)(size_t); /* may be NULL */
	int  (*set_device)(int32_t); /* may be NULL */
	int  (*device_count)(void);  /* may be NULL */
	int  (*arc_round_x)(pga_ctx_t *, int32_t, int32_t, const struct pga_loop_xchg_s *, int32_t *, int32_t *, int64_t *); /* may be NULL */
	int  (*copy_gbps)(size_t, int32_t, double *); /* may be NULL */
	int  (*warm)(void); /* may be NULL */
	int  (*reserve)(int64_t, int64_t, int32_t, int32_t, int32_t, int64_t); /* may be NULL */
	int  (*stage)(const void *, size_t); /* may be NULL */
	void (*stage_drop)(const void *);    /* may be NULL */
	int  (*call_bubbles)(const pga_call_in_t *, pga_call_out_t *); /* may be NULL: the host driver then runs the same step itself */
	int  (*pan_curves)(const pga_curves_in_t *, pga_curves_out_t *); /* may be NULL: the host driver then runs the same step itself */
	int  (*pan_shared)(const pga_shared_in_t *, pga_shared_out_t *); /* may be NULL: the host driver then runs the same step itself */
	int  (*pan_assoc)(const pga_assoc_in_t *, pga_assoc_out_t *); /* may be NULL: the host driver then runs the same step itself */
	int  (*pan_trait)(const pga_trait_in_t *, pga_trait_out_t *); /* may be NULL: the host driver then runs the same step itself */
	int  (*pan_join)(const pga_join_in_t *, pga_join_out_t *); /* may be NULL: the host driver then runs the same step itself */
	int  (*pan_boot)(const pga_boot_in_t *, pga_boot_out_t *); /* may be NULL: the host driver then runs the same step itself */
	int  (*pan_pairs)(const pga_pairs_in_t *, pga_pairs_out_t *); /* may be NULL: the host driver then runs the same step itself */
	int  (*pan_qtrait)(const pga_qtrait_in_t *, pga_qtrait_out_t *); /* may be NULL: the host driver then runs the same step itself */
	int  (*pan_medoids)(const pga_medoids_in_t *, pga_medoids_out_t *); /* may be NULL: the host driver then runs the same step itself */
	int  (*pan_permanova)(const pga_permanova_in_t *, pga_permanova_out_t *); /* may be NULL: the host driver then runs the same step itself */
	int  (*pan_mantel)(const pga_mantel_in_t *, pga_mantel_out_t *); /* may be NULL: the host driver then runs the same step itself */
	int  (*final_arcs)(pga_ctx_t *, const void **, int64_t *); /* may be NULL.  The final arc table of a branch_loop that ran with final_on: host view, count; 1 = not available */
	int  (*pan_gainloss)(const pga_gainloss_in_t *, pga_gainloss_out_t *); /* may be NULL: the host driver then runs the same step itself */
	int  (*pan_coevo)(const pga_coevo_in_t *, pga_coevo_out_t *); /* may be NULL: the host driver then runs the same step itself */
	int  (*post_front)(pga_ctx_t *, double, int32_t, int32_t, const int32_t **); /* may be NULL: the host driver then computes the representatives itself and calls post_apply */
	int  (*pan_phylosig)(const pga_phylosig_in_t *, pga_phylosig_out_t *); /* may be NULL: the host driver then runs the same step itself */
	int  (*pan_pcoa)(const pga_pcoa_in_t *, pga_pcoa_out_t *); /* may be NULL: the host driver then runs a second implementation (Jacobi on the dense B) */
	int  (*pan_glm)(const pga_glm_in_t *, pga_glm_out_t *); /* may be NULL: the host driver then runs a second implementation (the set bits walked in fp64) */
	int  (*pan_rates)(const pga_rates_in_t *, pga_rates_out_t *); /* may be NULL: the host driver then runs a second implementation (plain loops node by node in join order) */
} pga_backend_t;

const pga_backend_t *pga_backend(void);

/* The branch-filter rounds of pg_graph_gen (graph.c:300-314) without the host in between.  Behind a deferred arc round of a run
 * that is not sharded (arc_round_local(seg_cnt = NULL)), rounds r = 0 .. n_round-1 are queued back to back:
 *   pg_mark_branch_flt_arc (rep_pos, branch_pairs, branch_decide), pg_mark_branch_flt_hit + PG_SET_FILTER(weak_br == 2),
 *   for r > 0 pg_flt_high_occ's three tests with max_tot_cnt[r] / max_degree[r] / max_dist_loci[r] (graph.c:226-258) and
 *   PG_SET_FILTER(vtx == 0), and -- except after the last round -- the next pg_gen_arc.
 * A deleted segment is not renumbered away: its gene loses its vertex (g2s = -1), its two vertices keep their numbers and
 * simply have no arcs from then on (renumbering is monotone, so the order of every arc list, pair list and group number --
 * all the rounds look at -- is the same with the holes as without).  seg_alive[n_seg] (host) tells the caller which
 * segments are left; it renumbers them, hands the new g2s over (flag_vtx) and runs the arc round the loop left out.
 * ONE wait, at the end.  Returns 0; 1 = something the queued rounds could not handle happened on the way (a hub gene
 * overflowed its LDS table, the pair list its capacity): the shard's state is then undefined and the caller repeats the
 * run with host-driven rounds; 2 = not applicable here (nothing was queued); 3 (sharded form only) = an exchange buffer
 * was too small: state undefined as with 1, but the capacities have been raised and a later run can queue its rounds again.
 * 4 (unsharded form) = a pair list was longer than the room the loop had reserved, and nothing else went wrong: state undefined as with 1,
 * the room has been made (up to 2^27 pairs) and the caller repeats the run WITH queued rounds.
 *
 * Sharded form (x != NULL): behind pga_arc_set_current (the merged table of a host-driven round), every rank queues the same
 * rounds; where the host-driven route exchanges (graph_driver.cpp gen_arc / mark_branch_flt_arc) the backend calls x's two
 * collectives between its kernels -- per round ONE all-gather (every rank's slot: arc count, segment counters, arc table; the
 * tables are merged by key on the device, counts never leave it) and ONE all-reduce (the n_local counts of the round's pair
 * list, at a capacity all ranks share), plus one small all-reduce at the end that makes the return value collective.  A
 * callback returns when its collective is ORDERED with the context's stream: enqueued on it (RCCL on pga_active_stream), or
 * completed after the callee waited for the stream itself.  Every rank must call with the same n_round, capacities follow
 * from values all ranks share (arc_cap_hint: the largest local arc table of the last host-driven round, over all ranks). */
typedef struct pga_loop_xchg_s {
	void *user;
	int32_t rank, world;
	int64_t arc_cap_hint;
	int (*allreduce_i32_sum)(void *user, void *buf, int64_t count);                  /* in place, device memory */
	int (*allgather)(void *user, const void *in, void *out, int64_t bytes_per_rank); /* out: world slots, rank order */
} pga_loop_xchg_t;
/* Page-locked host memory the backend keeps between contexts (mailboxes, staging areas): give back what exceeds keep_bytes. */
void pga_host_trim(size_t keep_bytes);
/* the HIP device of this process (before the first context); the number of visible devices */
int pga_set_device(int32_t device);
int pga_device_count(void);
/* Measurement support (SURVEY.md 8d asks for a copy kernel beside the spec figure): the bandwidth, GB/s of read + write, that a
 * 16-byte-per-lane copy of `bytes` reaches on the current device; best of `reps`. */
int pga_copy_gbps(size_t bytes, int32_t reps, double *gbps);
/* Bring the HIP runtime up and load this library's code object (a first launch does both, ~0.1-0.3 s): a command line calls it on a
 * helper thread while its PAF files are parsed, so that the first pga_create finds the device ready. */
int pga_warm(void);

typedef struct pga_branch_par_s {
	double branch_diff, branch_diff_dist, branch_diff_cut; int32_t local_dist, local_count, frag_mode, use_ori;
	/* pre_on != 0 (unsharded form only): the deferred arc round behind which the loop is called is graph 1's (graph.c:291), and the loop
	 * starts with graph 2's pg_flt_high_occ (graph.c:294-295: its tests with these three limits, n_dist_loci still 0) + the next
	 * pg_gen_arc (graph.c:296) before round 0 -- deletions as holes, like those of the rounds */
	int32_t pre_on, pre_max_tot_cnt, pre_max_degree, pre_max_dist_loci;
	/* final_on != 0 (unsharded form only): n_round = ALL the rounds, and the arc round behind the last one (graph.c:313 of round
	 * n-1, the graph that is written) is queued as well.  seg_cnt[2 n_seg] (graph.c:125-126 of that round) and n_dist_loci[2 n_seg]
	 * (branch.c:90 of the last branch step) come back with seg_alive, all in the numbering the loop was entered with; the table
	 * (arc_table) is in that numbering too: the caller renumbers segments and arcs (monotone, so every order stands).
	 * The loop also queues what follows it in pg_graph_gen before its one wait: PG_SET_FILTER(shadow) of graph.c:316 (the caller's
	 * set_filter(PGA_FLT_SHADOW) right behind the loop is then a no-op) and the table in its FINAL form -- pg_arc_t records with the
	 * segments renumbered by seg_alive and the roundings of graph.c:170-172 applied -- which pga_final_arcs hands out.
	 * PANGENE_LOOP=notail: neither. */
	int32_t final_on;
} pga_branch_par_t;
/* pg_gen_arc (graph.c:87-177) of a sharded run with ONE wait: arc_round + the exchange + arc_merge + arc_set_current, every table
 * size left on the device; the ranks' tables travel in slots of a capacity all ranks share (the largest local table the shard has
 * seen, with a margin; x->arc_cap_hint before the backend has seen one).  seg_cnt[2 n_seg], deg[2 n_seg] (host) and *n_arc are the
 * global results; the merged table is the current one (arc_table).  Returns 1 on EVERY rank when the round is void on some rank (a
 * hub gene beyond its LDS table, a table beyond its slot): the caller repeats the round through arc_round (which then takes the sort
 * path, without a second sweep) and the host-driven exchange; 2 = not applicable (no capacity known, n_seg = 0): nothing happened. */
int pga_arc_round_x(pga_ctx_t *ctx, int32_t use_ori, int32_t n_seg, const pga_loop_xchg_t *x, int32_t *seg_cnt, int32_t *deg, int64_t *n_arc);
int pga_branch_loop(pga_ctx_t *ctx, int32_t n_round, const pga_branch_par_t *par, const int32_t *max_tot_cnt, const int32_t *max_degree,
                    const int32_t *max_dist_loci, uint8_t *seg_alive, const pga_loop_xchg_t *x, int32_t *seg_cnt /* final_on: [2 n_seg], else NULL */, int32_t *n_dist_loci /* likewise */);

/* The table a pga_branch_loop with final_on left in the backend's page-locked memory: *host_view = n_arc records laid out as pg_arc_t
 * (pangene.h:90-98: x with the renumbered segments, n_genome, tot_cnt, avg_dist, s1, s2, every other bit 0), sorted by x; valid until the
 * context's next arc round or loop.  No wait, no copy.  Returns 1 when there is no such table: the loop did not run with final_on or did
 * not return 0, PANGENE_LOOP=notail, the sharded form, or a table larger than the landing area (16 arcs per oriented vertex of the graph
 * the loop was entered with; PANGENE_FINAL_ARCS_CAP=n records) -- arc_table + the caller's own conversion is the general route. */
int pga_final_arcs(pga_ctx_t *ctx, const void **host_view, int64_t *n_arc);

/* pg_post_process's middle without the host: called right behind post_partials (a run that is not sharded: the sums are this shard's), it does what the driver
 * otherwise does between a fetch of the sums and post_apply -- n and avg_score_adj of every protein, the representative of every gene (the protein with the largest
 * key (sum score_adj << 32) + count, hit.c:205-217), the joint-pseudogene predicate of hit.c:176-181 with min_cnt = n_genome * min_vertex_ratio as the host computes
 * it (joint_pseudo = 0: PG_F_NO_JOINT_PSEUDO) -- and then post_apply's own step.  Nothing is fetched, nothing uploaded, nobody waits.
 * *host_view = page-locked words that hold, AFTER THE CALLER'S NEXT WAIT for the stream (a fetch, sync, vtx_partials, ...):
 *   [0] != 0: some gene has two proteins at its largest key.  Which of them the reference takes depends on its unstable sort, which the backend does not replay: the
 *       shard's state from post_apply on was computed with an arbitrary one of them, and the caller repeats the run from `begin` with its own representatives;
 *   [16 ..): max_score_ori[n_prot], n[n_prot], avg_score_adj[n_prot], then rep_pid[n_gene] (-1: a gene without proteins).
 * Valid until the context's next post_front. */
int pga_post_front(pga_ctx_t *ctx, double min_cnt, int32_t joint_pseudo, int32_t drop_sgl_exon, const int32_t **host_view);

/* Optional: run every kernel on this hipStream_t instead of the library's own stream (lets a host
 * framework order its collectives with the kernels without extra synchronisation). */
int pga_set_stream(pga_ctx_t *ctx, void *hip_stream);
/* The hipStream_t the live context runs on (collectives of a sharded run are enqueued on it). */
void *pga_active_stream(void);

/* Kernel timing hooks for bench.py: HIP events bracket every launch of the named kernel class on the
 * library's stream, from the first pga_timing_reset on.  which: 0 = "k1" (stage A sweep, the hit-filter+overlap kernel),
 * 1 = the pg_flt_ov_isoform sweep, 2 = the other pg_shadow sweeps, 3 = the whole of stage A (pga_begin + pga_ingest), 4 = host waits
 * (count only); with PANGENE_TIME_ROUNDS=1 in the environment at pga_timing_reset also 5 = every pg_gen_arc round (graph.c:87-177: sweep, walk,
 * temp arcs, collapse -- two more events per round, so for a pass that is not itself timed) and 6 = its walk scan alone.
 * which | (k + 1) << 8 selects the k-th timed launch of the class alone.  7 is not a timing: which build of K1 the sweeps of stage A and
 * pg_post_process run on this upload -- n_launch = 1 k_sweep (the tile's exon lists staged in LDS), 0 k_sweep_lean (read where they are),
 * -1 not decided yet; total_ms = the exons a tile would stage, as sampled (units = tiles sampled; 0 when PANGENE_SWEEP_LISTS fixed the choice). */
/* Optional, before pga_create: the device memory a shard of about this size will ask for (hits, exons, proteins, genes, genomes, words of
 * packed blocks), allocated now and kept for the pga_create that follows -- hipMalloc of tens of gigabytes takes seconds, and a reader
 * that knows its files' sizes can have it done while it parses (pg_read_paf_batch does).  Too small an estimate costs nothing but the
 * attempt; blocks nobody claims go back with pga_host_trim(0).  Safe to call from any thread. */
int pga_reserve(int64_t n_hit, int64_t n_exon, int32_t n_prot, int32_t n_gene, int32_t n_genome, int64_t raw_words);
/* Blocks on their way before there is a context (round 6; SURVEY 8(d): "device upload included").  The reader packs the genomes into slabs of page-locked host
 * memory (host_alloc) while later files are still parsed; a slab that is full and completely written is handed over here: its first `bytes` bytes are copied to a
 * device buffer of the library's on a stream of its own, and nothing waits.  pga_create() takes the blocks it finds inside such a slab from that copy (device to
 * device, behind the copy's event) instead of across the host link again.  The caller promises not to write to [host, host + bytes) until pga_stage_drop(host),
 * which it calls before the slab is reused or freed (it waits for a copy still in flight).  Safe to call from any thread; 0 or an error code -- a slab that was
 * not staged is simply uploaded by pga_create() as before. */
int pga_stage_h2d(const void *host, size_t bytes);
void pga_stage_drop(const void *host);
int pga_timing_reset(pga_ctx_t *ctx);
int pga_timing_get(pga_ctx_t *ctx, int32_t which, double *total_ms, int64_t *n_launch, int64_t *units);

#ifdef __cplusplus
}
#endif
#endif
