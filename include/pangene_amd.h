/*
 * pangene_amd.h -- public C surface of the MI355X-native pangene graph-construction path.
 *
 * Drop-in boundary.  The reference has no plugin/FFI layer; its boundary *is* pangene.h:126-141, called
 * by main.c:117-142 in a fixed order.  This header re-declares that surface with identical struct
 * layouts (sizes checked by tests/test_abi.py: opt 128, hit 88, exon 8, prot 32, gene 16, ctg 16,
 * genome 56, data 72, seg 32, arc 32, graph 56) and identical function names and argument meaning, so a
 * program written against pangene.h links against libpangene_amd.so unchanged.
 *
 *   entry point            replaces (reference file:line)
 *   pg_opt_init            option.c:6-26
 *   pg_data_init/destroy   read.c:10-32
 *   pg_read_paf            read.c:107-262   (parse only; the per-genome filters of read.c:243-260 are
 *                                            deferred to pg_post_process and run on the GPU -- exact,
 *                                            SURVEY.md 9.5; nothing can observe the difference because
 *                                            main.c calls pg_post_process next)
 *   pg_post_process        graph.c:7-32     (+ the deferred read.c:243-260) -> HIP kernels.  The hits are taken as pg_read_paf
 *                                            left them (each genome is packed for the device while the next file is parsed);
 *                                            a genome edited in between is packed again: the pack carries a signature over
 *                                            every field of every hit and exon it was made from, checked by pg_post_process
 *   pg_graph_init/gen/destroy graph.c:34-47, 280-322 -> HIP kernels + host round driver
 *   pg_write_bed/graph/walk format.c:113-225
 *   pg_read_list_dict, pg_dict_destroy  read.c:305-318, dict.c:38-49 (main.c:73-75,140-142 need them)
 *   pg_realtime/cputime/peakrss sys.c:117-140   (main.c:117,149 need them)
 *
 * Additions (not in the reference) are at the end: the exchange hook used to shard genomes across
 * GPUs/processes, id-only scanning of PAFs owned by another shard, and error reporting.
 */
#ifndef PANGENE_AMD_H
#define PANGENE_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PG_VERSION "1.1-r231-mi355x"

/* pg_opt_t::flag bits (values as in pangene.h:8-17) */
#define PG_F_WRITE_BED_RAW   0x1
#define PG_F_WRITE_BED_WALK  0x2
#define PG_F_WRITE_BED_FLAG  0x4
#define PG_F_WRITE_NO_WALK   0x8
#define PG_F_WRITE_VTX_SEL   0x10
#define PG_F_FRAG_MODE       0x20
#define PG_F_NO_JOINT_PSEUDO 0x40
#define PG_F_ORI_FOR_BRANCH  0x80
#define PG_F_CHECK_STRAND    0x100
#define PG_F_DROP_SGL_EXON   0x200

typedef struct { uint64_t x, y; } pg128_t;

/* options; layout of pangene.h:23-42 */
typedef struct {
	uint32_t flag;
	int32_t  gene_delim;          /* -d */
	double   min_prot_ratio;      /* -l */
	double   min_prot_iden;       /* -e */
	double   score_adj_coef;      /* -m */
	double   min_ov_ratio;        /* -f */
	double   min_vertex_ratio;    /* -p */
	double   branch_diff;         /* -b */
	double   branch_diff_dist;    /* -y */
	double   branch_diff_cut;     /* -B */
	int32_t  max_avg_occ;         /* -c */
	int32_t  max_degree;          /* -g */
	int32_t  max_dist_loci;       /* -r */
	int32_t  n_branch_flt;        /* -T */
	int32_t  min_arc_cnt;         /* -a */
	int32_t  local_dist;          /* -D */
	int32_t  local_count;         /* -C */
	void    *excl, *incl, *preferred; /* opaque name sets from pg_read_list_dict (-X -I -P) */
} pg_opt_t;

typedef struct { int32_t os, oe; } pg_exon_t;       /* exon [os,oe) relative to pg_hit_t::cs */

typedef struct {
	const char *name;
	int32_t len, gid;
	int32_t rep;
	int32_t n, avg_score_adj, max_score_ori;
} pg_prot_t;

typedef struct {
	const char *name;
	uint32_t len:30, preferred:1, included:1;
	int32_t rep_pid;
} pg_gene_t;

typedef struct {                                     /* 88 bytes; cs@64 cm@72 ce@80 */
	int32_t pid;
	int32_t qs, qe;
	int32_t cid;
	int32_t mlen, blen, lof;
	int32_t rank;
	int32_t score_ori, score_adj, score_dom;
	int32_t n_exon, off_exon;
	int32_t pid_dom, pid_dom0;
	uint32_t rev:1, flt:1, flt_iso_sub_self:1, flt_iso_ov:1, flt_chain:1, pseudo:1, vtx:1, shadow:1, rep:1, weak_br:2;
	int64_t cs, cm, ce;
} pg_hit_t;

typedef struct { const char *name; int64_t len; } pg_ctg_t;

typedef struct {
	int32_t n_ctg, m_ctg;   pg_ctg_t *ctg;
	int32_t n_hit, m_hit;   pg_hit_t *hit;
	int32_t n_exon, m_exon; pg_exon_t *exon;
	char *label;
} pg_genome_t;

typedef struct {
	void *d_ctg, *d_gene, *d_prot;
	int32_t n_genome, m_genome; pg_genome_t *genome;
	int32_t n_gene, m_gene;     pg_gene_t *gene;
	int32_t n_prot, m_prot;     pg_prot_t *prot;
} pg_data_t;

typedef struct {
	int32_t gid, n_dom, n_sub;
	int32_t n_genome;
	int32_t tot_cnt;
	uint32_t del:1, dummy:31;
	int32_t n_dist_loci[2];
} pg_seg_t;

typedef struct {
	uint64_t x;                  /* v<<32|w with v = segment<<1|strand */
	int32_t n_genome;
	int32_t tot_cnt;
	int32_t avg_dist;
	int32_t s1, s2;
	uint32_t del:1, weak_br:2, dummy:29;
} pg_arc_t;

typedef struct {
	pg_data_t *d;
	int32_t *g2s;
	int32_t n_seg, m_seg; pg_seg_t *seg;
	int32_t n_arc, m_arc; pg_arc_t *arc;
	uint64_t *idx;
} pg_graph_t;

extern int pg_verbose;

void       pg_opt_init(pg_opt_t *opt);
pg_data_t *pg_data_init(void);
void       pg_data_destroy(pg_data_t *d);
int32_t    pg_read_paf(const pg_opt_t *opt, pg_data_t *d, const char *fn);   /* -1 if fn cannot be opened */
void       pg_post_process(const pg_opt_t *opt, pg_data_t *d);
pg_graph_t *pg_graph_init(pg_data_t *d);
void       pg_graph_gen(const pg_opt_t *opt, pg_graph_t *q);
void       pg_graph_destroy(pg_graph_t *g);
void       pg_write_bed(const pg_data_t *d, int32_t is_walk);
void       pg_write_graph(const pg_graph_t *g);
void       pg_write_walk(pg_graph_t *g);
void      *pg_read_list_dict(const char *o);
void       pg_dict_destroy(void *h);
/* private in the reference too (pgpriv.h, sys.c:117-140) but called by main.c:117,149 */
double     pg_realtime(void);   /* seconds since the first call */
double     pg_cputime(void);    /* user + system CPU seconds */
long       pg_peakrss(void);    /* bytes */

/* ---------------------------------------------------------------------------------------------
 * Additions
 * ------------------------------------------------------------------------------------------- */

/* pangene.js `gfa2matrix` (pangene.js:1168-1247), the gene x assembly presence / copy-number matrix:
 * pg_write_matrix prints it for the graph in memory (after pg_graph_gen; the per-hit reduction runs on the GPU),
 * pg_gfa2matrix_file for any GFA file, plain or gzipped, exactly as the script does (clstr_fn: optional CD-HIT cluster
 * file, option -d there; print_cd: its -p).  Output: "Gene<TAB>asm..." then one row per segment. */
void pg_write_matrix(pg_graph_t *g, int32_t copy_number);
int  pg_gfa2matrix_file(const char *gfa_fn, int32_t copy_number, const char *clstr_fn, int32_t print_cd);

/* pangene.js `call` (pangene.js:93-392, 440-980; version 1.1-r231), bubble calling with the alleles the walks take through each
 * bubble, byte for byte.  The options are the script's: max_ext (-m, default 100; <0 never happens there, INT32_MAX stands for
 * its NaN), ignore_walk -w, use_pst -p, add_super -s, ref -r (NULL: none), and the outputs -b (Bandage CSV), -e (cycle
 * equivalence), -d (DFS); with none of the three the bubble report ("CC" header, FB / BB / AL lines) is printed.  The walk side
 * (which walks pass a bubble, alleles, genes) runs on the backend (pga_call_bubbles).
 * pg_call_file reads a GFA file, plain or gzipped, as the script does; it returns 0, -1 when the file cannot be opened, -2 when
 * the script would have stopped with an error ("Wrong!" for a GFA that lists links in one direction only, "DFS bug"): one line
 * on stderr then and nothing on the output.  pg_write_call does the same for the graph in memory after pg_graph_gen: the
 * segments, links and walks pg_write_graph / pg_write_walk would print, taken from the arrays behind them. */
typedef struct {
	int32_t max_ext, ignore_walk, use_pst, add_super;
	int32_t print_bandage, print_cec, print_dfs;
	const char *ref;
} pg_call_opt_t;
void pg_call_opt_init(pg_call_opt_t *o);
int  pg_call_file(const char *gfa_fn, const pg_call_opt_t *o);
void pg_write_call(pg_graph_t *g, const pg_call_opt_t *o);

/* Pangenome accumulation (rarefaction) curves: pan, core, new and unique genes as the assemblies are added in n_perm orders.  Genes
 * are the rows and assemblies the columns of the gfa2matrix matrix, a gene counts as present where its entry is > 0.  Order 0 is
 * the column order; order p >= 1 is a Fisher-Yates shuffle driven by splitmix64 seeded with (seed << 32) | p (README).  For the
 * first k columns of an order: pan = genes present in at least one, core = in all, new = in the k-th and none before, unique = in
 * exactly one.  The counting runs on the backend (pga_pan_curves).  Output: "Stat<TAB>Perm<TAB>1 ... n_asm", then one line
 * "stat<TAB>p<TAB>v1 ..." per statistic and order: all pan lines (p = 0 .. n_perm-1), then core, new and unique.
 * pg_write_curves: the graph in memory after pg_graph_gen (the matrix pg_write_matrix prints); pg_curves_file: a GFA file, plain or
 * gzipped (returns 0, -1 when the file cannot be opened); pg_pan_curves: any presence matrix, row-major uint8 [n_gene][n_asm],
 * out = int32 [4][n_perm][n_asm] (pan, core, new, unique); returns 0 or a PGA_ERR_* code. */
typedef struct {
	int32_t n_perm; /* orders, the input order first [10] */
	uint32_t seed;  /* [11] */
} pg_curves_opt_t;
void pg_curves_opt_init(pg_curves_opt_t *o);
void pg_write_curves(pg_graph_t *g, const pg_curves_opt_t *o);
int  pg_curves_file(const char *gfa_fn, const pg_curves_opt_t *o);
int  pg_pan_curves(const uint8_t *presence, int32_t n_gene, int32_t n_asm, const pg_curves_opt_t *o, int32_t *out);

/* Pairwise distances of the assemblies.  Each assembly is a set of items: its genes (type PG_DIST_GENE: the gfa2matrix entry is > 0)
 * or the gene adjacencies its walks traverse (PG_DIST_ADJ: consecutive steps (u, v) of one W-line, steps = segment * 2 + reverse,
 * unknown segments dropped, key min((u, v), (v ^ 1, u ^ 1)) so that >a>b and <b<a are one adjacency).  S[i][j] = items shared by i
 * and j (the backend's pga_pan_shared); with n_i = S[i][i]: jaccard = 1 - S[i][j] / (n_i + n_j - S[i][j]) (0 when the union is
 * empty, printed %.6f), shared = S[i][j], diff = n_i + n_j - 2 S[i][j].  Columns in gfa2matrix order and names (sample#hap).
 * Output, tab-separated: "Asm" and the names, then per assembly its name and its row; phylip: the count on the first line and the
 * rows without the header.  pg_dist_file: a GFA file, plain or gzipped (0, -1 when it cannot be opened, -2 on a backend error);
 * pg_write_dist: the graph in memory after pg_graph_gen; pg_pan_shared: any presence matrix, row-major uint8 [n_item][n_asm],
 * shared = int32 [n_asm][n_asm]; pg_pan_dist: the same, out = double [n_asm][n_asm] of the metric; both return 0 or PGA_ERR_*. */
enum { PG_DIST_GENE = 0, PG_DIST_ADJ = 1 };
enum { PG_DIST_JACCARD = 0, PG_DIST_SHARED = 1, PG_DIST_DIFF = 2 };
typedef struct {
	int32_t type;   /* PG_DIST_GENE or PG_DIST_ADJ [gene] */
	int32_t metric; /* PG_DIST_JACCARD, PG_DIST_SHARED or PG_DIST_DIFF [jaccard] */
	int32_t phylip; /* relaxed PHYLIP layout [0] */
} pg_dist_opt_t;
void pg_dist_opt_init(pg_dist_opt_t *o);
int  pg_dist_file(const char *gfa_fn, const pg_dist_opt_t *o);
void pg_write_dist(pg_graph_t *g, const pg_dist_opt_t *o);
int  pg_pan_shared(const uint8_t *presence, int32_t n_item, int32_t n_asm, int32_t *shared);
int  pg_pan_dist(const uint8_t *presence, int32_t n_item, int32_t n_asm, int32_t metric, double *out);

/* A tree of the assemblies from the distances above (DESIGN.md section 8 "Trees" holds the definition).  The jaccard or diff distances
 * become integers q = distance * 2^F (jaccard: F = 20, q = ((2^21)(u - s) + u) / (2u) with u = n_i + n_j - s, 0 for an empty union;
 * diff: q = (n_i + n_j - 2s) << F, F = min(20, 29 - bitlength(largest difference)), PGA_ERR_RANGE when F < 0; shared is not a
 * distance and is refused).  Neighbour-joining (PG_TREE_NJ) or UPGMA (PG_TREE_UPGMA) then joins slots 0 .. A - 1 in 64-bit integer
 * arithmetic: ties go to the smallest slot i, then the smallest j, slot i stands for the new node and slot j retires.  A join is one
 * record of six int64: NJ (i, j, d_ij, R_i, R_j, r), with R the row sums over the r live slots, and at r = 3 the closing record
 * (x, y, z, d_xy, d_xz, d_yz): A - 2 records; UPGMA (i, j, d_ij, n_i, n_j, r) with n the leaves below a slot: A - 1 records.
 * A distance that reaches 2^30 in size on the way: PGA_ERR_RANGE.  The records come from the backend's pga_pan_join.
 * Output: one Newick line; leaves are the gfa2matrix names (sample#hap), single-quoted when they hold one of (),:;[]' or white space;
 * branch lengths in distance units, %.6f; an NJ tree is unrooted (a trifurcation at the last record) and its negative branch lengths
 * are printed as they come; a UPGMA tree is rooted and ultrametric up to the integer floors.  One assembly: "(name);", two:
 * "(a:h,b:h);" with h half their distance, none: ";".
 * pg_tree_file: a GFA file (0, -1 when it cannot be opened, -2 on a backend or range error); pg_write_tree: the graph in memory after
 * pg_graph_gen; pg_pan_join: q = int32 [n][n], symmetric with a zero diagonal (PGA_ERR_ARG otherwise), every entry below 2^29 in size
 * (PGA_ERR_RANGE), 3 <= n <= 65 535, rec = room for n - 2 (NJ) or n - 1 (UPGMA) records; pg_pan_tree: a presence matrix, row-major
 * uint8 [n_item][n_asm] with n_asm >= 3, through the shared-item counts to the records, *frac_bits = F; both return 0 or PGA_ERR_*.
 * Bootstrap support (DESIGN.md section 8 "Bootstrap"): replicate b = 1 .. n_boot draws as many items as there are, with replacement --
 * x0 = mix64((seed << 32) | b) with the mix64 of pg_curves_*, draw t = 0 .. M - 1 is item mix64(x0 + (t + 1) * 0x9E3779B97F4A7C15) % M --
 * and is joined like the tree itself, distances, F and tie rule included (the backend's pga_pan_boot).  With C(s) the leaves below the
 * node of join s: an NJ join s < A - 3 is supported by a replicate that has a join with the same leaves or with all the others (the
 * same split of the unrooted tree), a UPGMA join s < A - 2 by one with the same leaves; count[s] = the supporting replicates, and
 * n_boot for NJ's closing record and UPGMA's root.  With n_boot > 0 the node of join s is printed "(...,...)P", P = the per cent of
 * count[s] rounded half up; the trifurcation and the root carry no label; n_boot = 0 prints the plain tree.  A range error in any
 * replicate is PGA_ERR_RANGE for the whole call.  pg_pan_boot: the records of the tree as pg_pan_tree returns them and count[n_rec];
 * pg_pan_boot_records: the records of replicates first .. first + n - 1 (first >= 1) as rec_out[n][n_rec][6]. */
enum { PG_TREE_NJ = 0, PG_TREE_UPGMA = 1 };
typedef struct {
	int32_t type;   /* PG_DIST_GENE or PG_DIST_ADJ [gene] */
	int32_t metric; /* PG_DIST_JACCARD or PG_DIST_DIFF [jaccard] */
	int32_t method; /* PG_TREE_NJ or PG_TREE_UPGMA [nj] */
	int32_t n_boot; /* bootstrap replicates; 0: none [0] */
	uint32_t seed;  /* seed of their draws [0] */
} pg_tree_opt_t;
void pg_tree_opt_init(pg_tree_opt_t *o);
int  pg_tree_file(const char *gfa_fn, const pg_tree_opt_t *o);
void pg_write_tree(pg_graph_t *g, const pg_tree_opt_t *o);
int  pg_pan_join(const int32_t *q, int32_t n, int32_t method, int64_t *rec);
int  pg_pan_tree(const uint8_t *presence, int32_t n_item, int32_t n_asm, int32_t metric, int32_t method, int64_t *rec, int32_t *frac_bits);
int  pg_pan_boot(const uint8_t *presence, int32_t n_item, int32_t n_asm, int32_t metric, int32_t method, int32_t n_boot, uint32_t seed, int64_t *rec,
                 int32_t *frac_bits, int32_t *count);
int  pg_pan_boot_records(const uint8_t *presence, int32_t n_item, int32_t n_asm, int32_t metric, int32_t method, uint32_t seed, int32_t first, int32_t n,
                         int64_t *rec_out);

/* Clusters of the assemblies: k-medoids (PAM) over the fixed-point distances of pg_tree_* (DESIGN.md section 8 "Clusters" holds the
 * definition; jaccard or diff, shared is refused).  With TD(M) the sum over the assemblies of their distance to the nearest medoid of M:
 * BUILD picks k medoids one by one, each the assembly that lowers TD the most (ties to the smallest index); SWAP then exchanges, at most
 * max_iter times, the pair (x not a medoid, m a medoid) with the smallest TD(M - m + x) - TD(M), ties to the smallest x and then the
 * smallest m, and stops -- converged -- when no exchange lowers TD.  Integers throughout.  The medoids in ascending order are clusters
 * 0 .. k - 1 (printed 1 .. k); a medoid belongs to its own cluster, any other assembly to the medoid with the smallest (distance, index).
 * The silhouette of assembly o of cluster c comes from sums[o][c'] = the sum of its distances to the members of c': a = sums[o][c] /
 * (size_c - 1), b = the smallest sums[o][c'] / size_c' over c' != c (compared by cross-multiplication, the first of equal ones),
 * s = (b - a) / max(a, b) as one double division of the cross-products; 0 in a cluster of one and where a = b = 0.  A mean silhouette is
 * the sum in assembly order, in double, over the count.  k_lo .. k_hi are run independently; the assignment is printed for the k with the
 * largest mean silhouette, ties to the smallest k.
 * Output, tab-separated, three blocks, each behind a header line that starts with '#':
 *   K  k TD mean_sil swaps converged        one line per k of the range
 *   C  cluster medoid size mean_sil         the chosen k, clusters 1 .. k, medoid = the assembly's name
 *   A  assembly cluster medoid dist sil     the assemblies in gfa2matrix order
 * TD and dist in distance units as %.6f, silhouettes as %.4f.  A k that does not converge within max_iter: a note on stderr, converged 0.
 * Fewer than 3 assemblies, or a k outside [2, assemblies - 1]: an error, nothing is printed.
 * pg_cluster_file: a GFA file (0, -1 when it cannot be opened, -2 on any other error); pg_write_cluster: the graph in memory after
 * pg_graph_gen (pg_last_error() is PGA_ERR_ARG, -3, after such a refusal, and the command line then exits with status 1 as it does for
 * a file).  pg_pan_medoids: q = int32 [n][n], symmetric, zero diagonal, no negative entry (PGA_ERR_ARG otherwise), every entry below
 * 2^29 (PGA_ERR_RANGE), 3 <= n <= 65 535, 2 <= k <= min(n - 1, 1 024), max_iter >= 0; fills medoid[k], label[n], dist[n], size[k],
 * sums[n][k], td, n_swap, converged and the first rec_cap of the *n_rec = k + n_swap records rec[.][3]: BUILD's (x, -1, gain), then the
 * swaps' (x, m, delta).  pg_pan_cluster: a presence matrix, row-major uint8 [n_item][n_asm], through the shared-item counts and the
 * fixed-point distances (*frac_bits = F) to the same results.  Both return 0 or PGA_ERR_*.  The runs come from the backend's
 * pga_pan_medoids. */
typedef struct {
	int32_t type;     /* PG_DIST_GENE or PG_DIST_ADJ [gene] */
	int32_t metric;   /* PG_DIST_JACCARD or PG_DIST_DIFF [jaccard] */
	int32_t k_lo;     /* the smallest k of the range, >= 2 [2] */
	int32_t k_hi;     /* the largest, >= k_lo [2] */
	int32_t max_iter; /* swap iterations per k at the most [1000] */
} pg_cluster_opt_t;
void pg_cluster_opt_init(pg_cluster_opt_t *o);
int  pg_cluster_file(const char *gfa_fn, const pg_cluster_opt_t *o);
void pg_write_cluster(pg_graph_t *g, const pg_cluster_opt_t *o);
int  pg_pan_medoids(const int32_t *q, int32_t n, int32_t k, int32_t max_iter, int32_t *medoid, int32_t *label, int32_t *dist, int32_t *size, int64_t *sums, int64_t *rec,
                    int32_t rec_cap, int32_t *n_rec, int32_t *n_swap, int64_t *td, int32_t *converged);
int  pg_pan_cluster(const uint8_t *presence, int32_t n_item, int32_t n_asm, int32_t metric, int32_t k, int32_t max_iter, int32_t *medoid, int32_t *label, int32_t *dist,
                    int32_t *size, int64_t *sums, int64_t *rec, int32_t rec_cap, int32_t *n_rec, int32_t *n_swap, int64_t *td, int32_t *converged, int32_t *frac_bits);

/* Gene associations: which genes travel together over the assemblies and which exclude each other.  Over the presence matrix of
 * gfa2matrix (gene g is in assembly a when its entry is > 0; rows in segment order), with A assemblies, a = |B_g|, b = |B_h|,
 * s = |B_g & B_h|: V_g = a (A - a), D = s A - a b, phi(g, h) = D / sqrt(V_g V_h).  Gene g is eligible when min(a, A - a) >= min_count
 * (core genes and genes seen nowhere have V = 0; with the default 2 singletons are out too).  min_phi is read as per-mille,
 * p = floor(1000 min_phi + 0.5), and a pair g < h of eligible genes is selected when 10^6 D^2 >= p^2 V_g V_h -- decided in 128-bit
 * integers, never in floating point -- and the sign of D is asked for (D = 0 counts as positive).  More than max_pair selected pairs
 * is an error (PGA_ERR_RANGE; the message names the number that passed).  Output, tab-separated: "GeneA GeneB nA nB nAB phi", then
 * one line per selected pair in ascending (row of A, row of B); phi = (double)D / sqrt((double)V_g * (double)V_h) as %.4f.
 * pg_assoc_file: a GFA file, plain or gzipped (0, -1 when it cannot be opened, -2 on a backend error or bad options);
 * pg_write_assoc: the graph in memory after pg_graph_gen; pg_pan_assoc: any presence matrix, row-major uint8 [n_gene][n_asm]: writes
 * the first cap selected pairs as pair[.][3] = (g, h, s) and returns the number selected, or a negative PGA_ERR_*.
 * n_asm <= 16 777 215. */
enum { PG_ASSOC_BOTH = 0, PG_ASSOC_POS = 1, PG_ASSOC_NEG = 2 };
typedef struct {
	double  min_phi;   /* smallest |phi| of a selected pair, in [0, 1], read as per-mille [0.8] */
	int32_t min_count; /* a gene is eligible when min(a, A - a) >= min_count; >= 1 [2] */
	int32_t sign;      /* PG_ASSOC_BOTH, PG_ASSOC_POS or PG_ASSOC_NEG [both] */
	int64_t max_pair;  /* more selected pairs than this is an error [16 777 216] */
} pg_assoc_opt_t;
void    pg_assoc_opt_init(pg_assoc_opt_t *o);
int     pg_assoc_file(const char *gfa_fn, const pg_assoc_opt_t *o);
void    pg_write_assoc(pg_graph_t *g, const pg_assoc_opt_t *o);
int64_t pg_pan_assoc(const uint8_t *presence, int32_t n_gene, int32_t n_asm, const pg_assoc_opt_t *o, int32_t *pair, int64_t cap);

/* Gene-trait association: which genes go with a binary phenotype of the assemblies (the pan-GWAS question).  Presence as for
 * pg_assoc_*.  The trait file (plain or gzipped) is tab-separated: a header line (any first field, then one trait name per column),
 * then per line an assembly name as gfa2matrix prints it and per trait 1, 0, or NA / empty (missing); lines starting with '#' after
 * the header and blank lines are skipped.  An assembly the file does not name is missing for every trait; a name the matrix does not
 * have, a repeated name, a wrong field count or another value is an error (the line number goes to stderr).  Per trait the columns
 * with a value are compacted, in matrix order, to N columns with labels y, t = sum y; a trait with t = 0 or t = N prints nothing.
 * For gene g: a = |B_g|, s = |B_g & y|, D = s N - a t, V_g = a (N - a), V_t = t (N - t); g is eligible when min(a, N - a) >= min_count.
 * Permutation p = 1 .. n_perm is y_p[r] = y[o_p[r]], o_p = order p of N columns exactly as pg_curves_* define it (seed as there);
 * s_p = |B_g & y_p|, D_p = s_p N - a t, k_g = #{p : |D_p| >= |D|} -- integers throughout (N <= 16 777 215).
 * Output, tab-separated: "Trait Gene N nT nG nTG phi p_fisher q_bh n_ge p_perm", one line per eligible gene and trait, traits in
 * file order, genes in row order: phi = D / sqrt(V_g V_t) as %.4f; p_fisher = the two-sided Fisher exact p (the sum of the
 * hypergeometric probabilities P(x) <= P(s) (1 + 1e-7), capped at 1) as %.3e; q_bh = Benjamini-Hochberg over the eligible genes of
 * the trait as %.3e; n_ge = k_g; p_perm = (k_g + 1) / (n_perm + 1) as %.6f (both NA with n_perm = 0).  Only lines with
 * p_fisher <= max_p are kept (q_bh is over all eligible genes all the same).
 * pg_trait_file: a GFA file and a trait file (0, -1 when the GFA cannot be opened, -2 on a backend error or bad options, -3 on a bad
 * trait file); pg_write_trait: the graph in memory after pg_graph_gen (errors: pg_last_error); pg_pan_trait: any presence matrix,
 * row-major uint8 [n_gene][n_asm], and labels, row-major int8 [n_trait][n_asm] (1, 0, -1 = missing): fills
 * out[5][n_trait][n_gene] = N, t, a, s, k (a = -1, s = k = 0 for a gene that is not eligible, and for every gene of a trait with
 * t = 0 or t = N) and returns 0 or a negative PGA_ERR_*.
 * Lineage-aware test (lineage = PG_LINEAGE_NJ or PG_LINEAGE_UPGMA; DESIGN.md section 8 "Lineage-aware trait test" holds the definition):
 * population structure confounds the counts above -- a gene and a trait that sit in the same clade give a tiny p_fisher from one
 * evolutionary event -- so every line gains the pairwise comparisons on a tree.  The tree is the one `pangene tree -t gene -m jaccard`
 * builds with that method over ALL assemblies of the matrix (NJ's closing trifurcation (x, y, z) read as ((x, y), z); the numbers below
 * belong to the unrooted tree).  A leaf with a trait value has the type (gene bit, y); a pair is two typed leaves that differ in both,
 * 11-00 supporting and 10-01 opposing; a pair set is a set of pairs whose tree paths share no vertex.  pairs = the size of a largest
 * pair set, supp / opp = the most supporting / opposing pairs a largest pair set can have (integers, the backend's pga_pan_pairs).
 * With `for` = supp when D >= 0 and opp otherwise, `against` the other, and P2(k, n) = min(1, 2 P(X >= max(k, n - k))) for X binomial
 * (n, 1/2), 1 for n = 0: p_pair_best = P2(for, pairs), p_pair_worst = P2(pairs - against, pairs).  Five more columns,
 * "pairs supp opp p_pair_best p_pair_worst", the p values as %.3e; without lineage the output is what it was.  At most 65 535 assemblies.
 * pg_pan_pairs: presence and labels as for pg_pan_trait, rec = the records of a tree over the n_asm assemblies as pg_pan_tree or
 * pg_pan_join return them for `method` (any such tree; not read when n_asm < 3: one leaf is a tree, two are one join): fills
 * out[3][n_trait][n_gene] = pairs, supp, opp and returns 0 or a negative PGA_ERR_* (records that name a slot out of range or a
 * retired one: PGA_ERR_ARG). */
enum { PG_LINEAGE_NONE = 0, PG_LINEAGE_NJ = 1, PG_LINEAGE_UPGMA = 2 };
typedef struct {
	int32_t  n_perm;    /* permutations; 0: none [1000] */
	uint32_t seed;      /* seed of the orders [11] */
	int32_t  min_count; /* a gene is eligible when min(a, N - a) >= min_count; >= 1 [1] */
	int32_t  reserved;
	double   max_p;     /* keep the lines with p_fisher <= max_p [1: all] */
	int32_t  lineage;   /* PG_LINEAGE_NONE, PG_LINEAGE_NJ or PG_LINEAGE_UPGMA: the pairwise comparisons on that tree [none] */
} pg_trait_opt_t;
void pg_trait_opt_init(pg_trait_opt_t *o);
int  pg_trait_file(const char *gfa_fn, const char *trait_fn, const pg_trait_opt_t *o);
void pg_write_trait(pg_graph_t *g, const char *trait_fn, const pg_trait_opt_t *o);
int  pg_pan_trait(const uint8_t *presence, const int8_t *labels, int32_t n_gene, int32_t n_asm, int32_t n_trait, const pg_trait_opt_t *o, int32_t *out);
int  pg_pan_pairs(const uint8_t *presence, const int8_t *labels, int32_t n_gene, int32_t n_asm, int32_t n_trait, const int64_t *rec, int32_t method, int32_t *out);

/* Quantitative traits: which genes go with a continuous phenotype of the assemblies (MIC values, growth rates, host ranges) -- the
 * Wilcoxon rank-sum (Mann-Whitney) test of the carriers of a gene against the others, with the permutation test of pg_trait_*.
 * The trait file has the shape pg_trait_* read (same line reader, header, '#' and blank lines, an assembly the file does not name
 * missing for every trait, the same errors with their line number); a field is NA or empty (missing) or a decimal number that strtod
 * consumes entirely with a finite result: nan, inf, an overflowing exponent such as 1e999, trailing characters and a bare '-' are errors.
 * Per trait the columns with a value are compacted, in matrix order, to N columns with values v.  Doubled midrank
 * r2[c] = 2 #{v < v_c} + #{v == v_c} + 1 (comparison of doubles: -0.0 equals 0.0); centred doubled rank c2[c] = r2[c] - (N + 1), so
 * sum c2 = 0 and |c2| <= N - 1.  A trait with N < 2 or with all values equal prints a note on stderr and no lines.
 * For gene g: a = |B_g| over the N columns, D = the sum of c2 over the columns of B_g = R2 - a (N + 1) with R2 the doubled rank sum of
 * the carriers; g is eligible when min(a, N - a) >= min_count.  Permutation p = 1 .. n_perm is c2_p[r] = c2[o_p[r]], o_p = order p of N
 * columns exactly as pg_trait_* and pg_curves_* define it (the same swap sequence applied to the value row; seed as there);
 * D_p = the sum of c2_p over B_g, k_g = #{p : |D_p| >= |D|} -- integers throughout.  On a file of 0s and 1s c2 is N - t for a 1 and
 * -t for a 0, so D = s N - a t, pg_trait_*'s D, and n_ge and p_perm equal pg_trait_*'s; D changes sign when every value is negated.
 * Output, tab-separated: "Trait Gene N nG U auc z p_wilcox q_bh n_ge p_perm", one line per eligible gene and trait, traits in file
 * order, genes in row order: nG = a; U = (D + a (N - a)) / 2, the carriers' Mann-Whitney U, as %.1f (half-integers are exact);
 * auc = U / (a (N - a)) as %.4f; z = D / sqrt(V) as %.4f with V = a (N - a) / 3 ((N + 1) - T / (N (N - 1))) and T the sum over the
 * tie groups of t^3 - t -- the tie-corrected normal approximation WITHOUT continuity correction; p_wilcox = erfc(|z| / sqrt 2) as
 * %.3e; q_bh = Benjamini-Hochberg over the eligible genes of the trait as %.3e; n_ge = k_g; p_perm = (k_g + 1) / (n_perm + 1) as %.6f
 * (both NA with n_perm = 0).  Only lines with p_wilcox <= max_p are kept (q_bh is over all eligible genes all the same).
 * At most 32 000 columns with a value per trait (PGA_ERR_RANGE): c2 then splits into two signed bytes and every sum fits int32.
 * pg_qtrait_file, pg_write_qtrait: as their trait twins, return codes included.  pg_pan_qtrait: any presence matrix, row-major uint8
 * [n_gene][n_asm], and values, row-major double [n_trait][n_asm] (NaN = missing; an infinite value is PGA_ERR_ARG): fills
 * out[4][n_trait][n_gene] = N, a, D, k (a = -1, D = k = 0 for a gene that is not eligible, and for every gene of a trait with N < 2 or
 * one value) and returns 0 or a negative PGA_ERR_*. */
typedef struct {
	int32_t  n_perm;    /* permutations; 0: none [1000] */
	uint32_t seed;      /* seed of the orders [11] */
	int32_t  min_count; /* a gene is eligible when min(a, N - a) >= min_count; >= 1 [1] */
	int32_t  reserved;
	double   max_p;     /* keep the lines with p_wilcox <= max_p [1: all] */
} pg_qtrait_opt_t;
void pg_qtrait_opt_init(pg_qtrait_opt_t *o);
int  pg_qtrait_file(const char *gfa_fn, const char *trait_fn, const pg_qtrait_opt_t *o);
void pg_write_qtrait(pg_graph_t *g, const char *trait_fn, const pg_qtrait_opt_t *o);
int  pg_pan_qtrait(const uint8_t *presence, const double *values, int32_t n_gene, int32_t n_asm, int32_t n_trait, const pg_qtrait_opt_t *o, int32_t *out);

/* PERMANOVA: do the two groups of a binary trait differ in gene content as a whole -- the two-group permutational multivariate analysis
 * of variance (Anderson 2001; adonis2 of vegan) over the fixed-point distances of pg_tree_* / pg_cluster_* (jaccard or diff with F
 * fraction bits; shared is refused), with the trait file and the permutations of pg_trait_*.  DESIGN.md section 8 "PERMANOVA" holds the
 * definition.  Per trait the columns with a value are compacted, in matrix order, to N columns with labels y, n1 = sum y, n0 = N - n1,
 * and qc is the N x N submatrix of the distances.  A trait with N < 3, n1 = 0 or n0 = 0, and a trait whose qc is all zero, prints a note
 * on stderr and no line.  Scaling: m = max qc, s the smallest s >= 0 with (m >> s)^2 N (N - 1) < 2^62, e = qc >> s, Fe = F - s,
 * w = e^2 (int64, zero diagonal).  r[i] = sum_j w[i][j], T = sum r, A(y) = sum over ordered pairs of y_i y_j w[i][j], B(y) = sum y_i r[i],
 * all below 2^62; SST = T / (2 N), SSW = A / (2 n1) + (T - 2 B + A) / (2 n0), and G(y) = N A - 2 n1 B (128 bits) orders SSW:
 * 2 n0 n1 SSW = G + n1 T.  Permutation p = 1 .. n_perm is y_p[r] = y[o_p[r]], o_p = order p of N columns exactly as pg_trait_* define it;
 * k = #{p : G(y_p) <= G(y)}, the permutations whose pseudo-F is at least the observed one (ties count) -- integers throughout.
 * Output, tab-separated: "Trait N n1 n0 Fbits SS_total SS_within F R2 n_ge p_perm", one line per trait in file order: Fbits = Fe;
 * SS_total = SST / 4^Fe and SS_within = SSW / 4^Fe as %.6f; F = (SST - SSW) (N - 2) / SSW as %.6f, inf when SSW = 0;
 * R2 = 1 - SSW / SST as %.4f; n_ge = k; p_perm = (k + 1) / (n_perm + 1) as %.6f, NA with n_perm = 0.  Each double is ONE long double
 * division of two 128-bit integers: with X = G + n1 T and Y = T n0 n1 - N X, SS_total = T / (2 N), SS_within = X / (2 n0 n1) (both then
 * scaled by the power of two), F = Y (N - 2) / (N X), R2 = Y / (T n0 n1).
 * At most 16 384 columns with a value per trait (PGA_ERR_RANGE).
 * pg_permanova_file, pg_write_permanova: as their trait twins, return codes included.  pg_pan_permanova: any fixed-point matrix
 * q = int32 [n][n] with o->frac_bits fraction bits, symmetric, zero diagonal, no negative entry (PGA_ERR_ARG otherwise), every entry
 * below 2^29 (PGA_ERR_RANGE), and labels, row-major int8 [n_trait][n] (1, 0, -1 = missing): fills out[n_trait][7] = N, n1, Fe, T, A, B, k
 * (Fe = T = A = B = 0 and k = -1 for a trait that prints no line) and returns 0 or a negative PGA_ERR_*.  pg_pan_permanova_presence: a
 * presence matrix, row-major uint8 [n_item][n_asm], through the shared-item counts and the fixed-point distances of o->metric
 * (*frac_bits = F; o->frac_bits is not read) to the same.  The sums and k come from the backend's pga_pan_permanova.
 * sizeof(pg_permanova_opt_t) is 20. */
typedef struct {
	int32_t  type;      /* PG_DIST_GENE or PG_DIST_ADJ [gene] */
	int32_t  metric;    /* PG_DIST_JACCARD or PG_DIST_DIFF [jaccard] */
	int32_t  n_perm;    /* permutations; 0: none [1000] */
	uint32_t seed;      /* seed of the orders [11] */
	int32_t  frac_bits; /* pg_pan_permanova only: the fraction bits F of q, 0 .. 30 [20] */
} pg_permanova_opt_t;
void pg_permanova_opt_init(pg_permanova_opt_t *o);
int  pg_permanova_file(const char *gfa_fn, const char *trait_fn, const pg_permanova_opt_t *o);
void pg_write_permanova(pg_graph_t *g, const char *trait_fn, const pg_permanova_opt_t *o);
int  pg_pan_permanova(const int32_t *q, int32_t n, const int8_t *labels, int32_t n_trait, const pg_permanova_opt_t *o, int64_t *out);
int  pg_pan_permanova_presence(const uint8_t *presence, int32_t n_item, int32_t n_asm, const int8_t *labels, int32_t n_trait, const pg_permanova_opt_t *o,
                               int64_t *out, int32_t *frac_bits);

/* Mantel test: do two distance matrices of the same assemblies agree -- does gene-order divergence track gene-content divergence, or
 * gene content an external distance (mantel of vegan).  DESIGN.md section 8 "Mantel test" holds the definition.  Inputs are two
 * fixed-point matrices qx, qy over the same N assemblies: symmetric, zero diagonal, entries in [0, 2^29).  Per matrix s is the smallest
 * s >= 0 with (max >> s)^2 N (N - 1) < 2^62 (the rule of pg_permanova_*, applied to each matrix on its own), a = qx >> sx, b = qy >> sy.
 * Over ordered pairs i != j, M = N (N - 1) of them: Sa = sum a, Sb = sum b, Saa = sum a^2, Sbb = sum b^2 and, for an order o of the
 * assemblies, Z(o) = sum a[i][j] b[o[i]][o[j]] -- all below 2^62.  Z is Z of the identity; permutation p = 1 .. n_perm uses o_p = order p of
 * N columns exactly as pg_trait_* define it; n_ge = #{p : Z_p >= Z}, n_le = #{p : Z_p <= Z}, ties in both -- integers throughout.
 * Output, tab-separated: "X Y N r n_ge n_le p_greater p_less" and one line: X and Y name the matrices (gene:jaccard, adj:diff, ..., or
 * file); with num = M Z - Sa Sb, va = M Saa - Sa^2, vb = M Sbb - Sb^2 (128 bits), r = (num / sqrtl(va)) / sqrtl(vb) in long double as
 * %.4f; p_greater = (n_ge + 1) / (n_perm + 1) and p_less = (n_le + 1) / (n_perm + 1) as %.6f, NA with n_perm = 0.  N < 3, va = 0 or
 * vb = 0: a note on stderr and the header only.  At most 16 384 assemblies (PGA_ERR_RANGE).
 * pg_mantel_file: X is the distance x_type:x_metric of the GFA file; Y is y_type:y_metric of the same file or, with mat_fn not NULL, the
 * matrix of that file in either form pg_dist_* print: the table ("Asm" and the names, then a name and its values per line) or relaxed
 * PHYLIP (a count line, then a name and its values per line), fields between blanks or tabs.  Values by strtod; F is the largest F in
 * [0, 20] with floor(vmax 2^F + 0.5) < 2^29 and q = floor(v 2^F + 0.5); r does not depend on F.  N is the assemblies both sides name, in
 * X's order; a name on one side only gets a note on stderr and is left out.  A matrix that is not square, a value that is not a finite
 * number >= 0, a diagonal value that is not 0, a name given twice and a matrix that is not symmetric after the conversion are errors that
 * name the file and the line.  Returns 0, -1 (the GFA file cannot be opened), -3 (a bad matrix file) or -2 (the backend's status is on
 * stderr).  pg_write_mantel: the same for the graph in memory; errors go to pg_last_error.
 * pg_pan_mantel: any two such matrices, int32 [n][n] each (PGA_ERR_ARG when one is not symmetric, has a diagonal entry that is not zero
 * or a negative entry, PGA_ERR_RANGE for an entry of 2^29 or more); only n_perm and seed of the options are read.  Fills
 * out[10] = N, sx, sy, Sa, Sb, Saa, Sbb, Z, n_ge, n_le (Z = 0 and n_ge = n_le = -1 for a pair that is not tested) and returns 0 or a
 * negative PGA_ERR_*.  Z and the counts come from the backend's pga_pan_mantel.  sizeof(pg_mantel_opt_t) is 24. */
typedef struct {
	int32_t  x_type, x_metric; /* X: PG_DIST_GENE or PG_DIST_ADJ, PG_DIST_JACCARD or PG_DIST_DIFF [gene:jaccard] */
	int32_t  y_type, y_metric; /* Y, unless a matrix file is given [adj:jaccard] */
	int32_t  n_perm;           /* permutations; 0: none [1000] */
	uint32_t seed;             /* seed of the orders [11] */
} pg_mantel_opt_t;
void pg_mantel_opt_init(pg_mantel_opt_t *o);
int  pg_mantel_file(const char *gfa_fn, const char *mat_fn, const pg_mantel_opt_t *o);
void pg_write_mantel(pg_graph_t *g, const char *mat_fn, const pg_mantel_opt_t *o);
int  pg_pan_mantel(const int32_t *qx, const int32_t *qy, int32_t n, const pg_mantel_opt_t *o, int64_t *out);

/* Gain and loss: on which branches of the assemblies' tree were items gained and lost, and which items changed hands many times --
 * ancestral gene-content reconstruction by parsimony (Wagner parsimony with a gain penalty, as in Count; Fitch parsimony when the two
 * costs are equal).  DESIGN.md section 8 "Gain and loss" holds the definition.  The items are the rows of the presence matrix (genes, or
 * with type PG_DIST_ADJ the gene adjacencies of the walks), the tree is the one pg_tree_* build with `metric` and `method` over all
 * assemblies.  The method defaults to UPGMA, which has a root; NJ is rooted at its closing record (x, y, z), read as ((x, y), z) as
 * pg_pan_pairs reads it, and gains and losses DEPEND on that reading (the cost does not when gain = loss = 1).  Nodes: leaves
 * 0 .. A - 1 in matrix order, join record s makes node A + s (NJ's closing record A + s and the root A + s + 1): 2 A - 1 nodes.
 * A gain (parent absent, child present) costs `gain`, a loss `loss`, 1 .. 255 each.  Per item, bottom-up: a leaf with bit b has
 * C[b] = 0, C[1 - b] = gain + loss; an inner node C[s] = the sum over its two children c of min(C_c[s], C_c[1 - s] + w(s)), w(0) = gain,
 * w(1) = loss.  Top-down: the root is present iff C[1] < C[0]; a child of a node in state s switches iff C_c[1 - s] + w(s) < C_c[s]
 * (mode PG_GAINLOSS_LATE: a tie keeps the parent's state, changes sit towards the tips) or <= (PG_GAINLOSS_EARLY: towards the root).
 * cost = gain * gains + loss * losses and is the smallest possible; a leaf's state is its bit.  Integers throughout.
 * Output, tab-separated.  out = PG_GAINLOSS_GENE: "Gene Present Cost Changes Gains Losses Root", one line per item in matrix order with
 * Changes = Gains + Losses >= min_changes (an adjacency is named by its two steps as a walk writes them, >a<b).  PG_GAINLOSS_NODE:
 * "Node Child1 Child2 Leaves Present Gains Losses": the leaves first under their assembly names with "." for both children, then the
 * joins in record order as @s with s = node - A; Present = the items in state 1 at the node, Gains and Losses those on the branch above
 * it, NA for the root.  No assemblies or no items: the header only.  At most 65 535 assemblies and 16 777 215 items (PGA_ERR_RANGE).
 * pg_gainloss_file: 0, -1 (the GFA file cannot be opened) or -2 (bad options, or the backend's status on stderr).  pg_write_gainloss: the
 * same for the graph in memory; errors go to pg_last_error.
 * pg_pan_gainloss: any presence matrix, row-major uint8 [n_item][n_asm], and any tree over the n_asm assemblies as the records pg_pan_tree
 * or pg_pan_join return for `method` (not read when n_asm < 3: one leaf is the root, two are one join); of the options only gain, loss
 * and mode are read.  Fills gene_out[n_item][5] = present, cost, gains, losses, root and node_out[2 n_asm - 1][3] = present, gains,
 * losses in node order (0 and 0 for the root) and returns 0 or a negative PGA_ERR_* (a NULL, an option out of range, records that name a
 * slot out of range or a retired one: PGA_ERR_ARG).  The two passes come from the backend's pga_pan_gainloss.
 * sizeof(pg_gainloss_opt_t) is 32. */
enum { PG_GAINLOSS_LATE = 0, PG_GAINLOSS_EARLY = 1 };
enum { PG_GAINLOSS_GENE = 0, PG_GAINLOSS_NODE = 1 };
typedef struct {
	int32_t type;        /* PG_DIST_GENE or PG_DIST_ADJ [gene] */
	int32_t metric;      /* PG_DIST_JACCARD or PG_DIST_DIFF [jaccard] */
	int32_t method;      /* PG_TREE_NJ or PG_TREE_UPGMA [upgma] */
	int32_t gain, loss;  /* the cost of a gain and of a loss, 1 .. 255 [1, 1] */
	int32_t mode;        /* PG_GAINLOSS_LATE or PG_GAINLOSS_EARLY [late] */
	int32_t out;         /* PG_GAINLOSS_GENE or PG_GAINLOSS_NODE [gene] */
	int32_t min_changes; /* the gene table keeps the items with Changes >= min_changes [0: all] */
} pg_gainloss_opt_t;
void pg_gainloss_opt_init(pg_gainloss_opt_t *o);
int  pg_gainloss_file(const char *gfa_fn, const pg_gainloss_opt_t *o);
void pg_write_gainloss(pg_graph_t *g, const pg_gainloss_opt_t *o);
int  pg_pan_gainloss(const uint8_t *presence, int32_t n_item, int32_t n_asm, const int64_t *rec, int32_t method, const pg_gainloss_opt_t *o, int32_t *gene_out,
                     int64_t *node_out);

/* Co-evolution: which item pairs were gained and lost on the same branches of the assemblies' tree -- the gene-gene association counted
 * over events on the tree instead of over tips (as Coinfinder's lineage correction and Goldfinder's simultaneous-event score do).
 * DESIGN.md section 8 "Co-evolution" holds the definition.  Items, tree and reconstruction are exactly those of pg_gainloss_* (type,
 * metric, method, gain, loss, mode).  Every node but the root has one branch above it: B = 2 A - 2.  Item i has the gain set G_i (node
 * present, parent absent) and the loss set L_i (the reverse); e_i = |G_i| + |L_i| is the Changes column of pg_gainloss_*.  For i < j:
 * same = |G_i & G_j| + |L_i & L_j|, opp = |G_i & L_j| + |L_i & G_j|, d = same - opp.  Items with e_i >= min_events are eligible; a pair of
 * eligible items is selected when 10^6 d^2 >= p^2 e_i e_j, p = floor(1000 min_r + 0.5), and the sign rule of pg_assoc_* holds (pos: d >= 0,
 * neg: d < 0).  Integers throughout; with B < 2^17 both sides stay below 2^54.
 * Output, tab-separated, in ascending (i, j): "ItemA ItemB nA nB eA eB same opp r p_hyper": the presence counts, the events, the two
 * counts, r = d / sqrt(eA eB) (%.4f) and p_hyper = P(X >= same + opp) for X ~ Hypergeometric(B, eA, eB) (%.3e), computed on the host for
 * the selected pairs.  It is a parsimony reading; under NJ it depends on the rooting; p_hyper treats the branches as exchangeable and is
 * a screening value.  A <= 1 or no items: the header only.  More than max_pair selected pairs is an error (PGA_ERR_RANGE, one line on
 * stderr, no table).  pg_coevo_file: 0, -1 (the GFA file cannot be opened) or -2; pg_write_coevo: errors go to pg_last_error.
 * pg_pan_coevo: any presence matrix [n_item][n_asm] and any tree as for pg_pan_gainloss; of the options type and metric are not read.
 * Fills events_out[n_item] = e_i (may be NULL) and the first min(cap, n) rows of pair_out[cap][4] = i, j, same, opp, and returns n, the
 * number selected, or a negative PGA_ERR_*.  The counting and the selection come from the backend's pga_pan_coevo.
 * sizeof(pg_coevo_opt_t) is 48. */
typedef struct {
	int32_t type;        /* PG_DIST_GENE or PG_DIST_ADJ [gene] */
	int32_t metric;      /* PG_DIST_JACCARD or PG_DIST_DIFF [jaccard] */
	int32_t method;      /* PG_TREE_NJ or PG_TREE_UPGMA [upgma] */
	int32_t gain, loss;  /* the cost of a gain and of a loss, 1 .. 255 [1, 1] */
	int32_t mode;        /* PG_GAINLOSS_LATE or PG_GAINLOSS_EARLY [late] */
	int32_t min_events;  /* an item is eligible when e_i >= min_events; >= 1 [2] */
	int32_t sign;        /* PG_ASSOC_BOTH, PG_ASSOC_POS or PG_ASSOC_NEG [both] */
	double  min_r;       /* smallest |r| of a selected pair, in [0, 1], read as per-mille [0.8] */
	int64_t max_pair;    /* more selected pairs than this is an error [16 777 216] */
} pg_coevo_opt_t;
void    pg_coevo_opt_init(pg_coevo_opt_t *o);
int     pg_coevo_file(const char *gfa_fn, const pg_coevo_opt_t *o);
void    pg_write_coevo(pg_graph_t *g, const pg_coevo_opt_t *o);
int64_t pg_pan_coevo(const uint8_t *presence, int32_t n_item, int32_t n_asm, const int64_t *rec, int32_t method, const pg_coevo_opt_t *o, int32_t *events_out,
                     int32_t *pair_out, int64_t cap);

/* Phylogenetic signal: does an item's presence follow the assemblies' tree?  The permutation tail probability of the parsimony length
 * (Faith & Cranston 1991) with the retention index beside it.  DESIGN.md section 8 "Phylogenetic signal" holds the definition.  Items,
 * tree and costs are those of pg_gainloss_* (type, metric, method, gain, loss); Cost = min(C0, C1) at the root does not depend on the
 * tie rule.  An item is tested when min(Present, A - Present) >= min_count; the classes are the distinct values of Present over the
 * tested items.  Replicate (n, p), p = 1 .. n_perm: with o_p the order every other permutation command uses for (A, seed, p), assembly x
 * is present iff o_p[x] < n; cost(n, p) is the Wagner cost of that tip set.  Per item n_le = #{p : cost(Present, p) <= Cost}, n_ge the
 * same with >=, p_signal = (1 + n_le) / (1 + n_perm) (small: fewer changes than chance, vertical), p_scatter = (1 + n_ge) / (1 + n_perm)
 * (small: more changes than chance), q_signal = Benjamini-Hochberg over p_signal of the tested items.  Per class Expect = the mean of
 * cost(n, p) over p.  MaxCost = min(n gain, (A - n) loss), the cost on an unresolved tree; RI = (MaxCost - Cost) / (MaxCost - min(gain,
 * loss)), NA when the denominator is 0.  Integers up to the printed ratios.
 * Output, tab-separated: "Gene Present Cost MaxCost Expect RI n_le n_ge p_signal p_scatter q_signal", one line per tested item in item
 * order with min(p_signal, p_scatter) <= max_p (q is computed before that filter); Expect %.3f, RI %.4f, the p and q values %.6f.
 * n_perm = 0 runs no permutation and prints NA for Expect, n_le, n_ge and the three p / q columns.  No assemblies, no items or no tested
 * item: the header only.  It is a parsimony reading; under NJ it depends on the rooting; the tips are treated as exchangeable.
 * pg_phylosig_file: 0, -1 (the GFA file cannot be opened) or -2; pg_write_phylosig: errors go to pg_last_error.
 * pg_pan_phylosig: any presence matrix [n_item][n_asm] and any tree as for pg_pan_gainloss; of the options gain, loss, n_perm, seed and
 * min_count are read.  Fills out_i32[n_item][5] = present, cost, tested (0 / 1), n_le, n_ge (0 and 0 for an item that is not tested) and
 * out_sum_i64[n_asm + 1], indexed by n: the sum over p of cost(n, p), 0 for a class that did not run.  Returns 0 or a negative PGA_ERR_*;
 * errors and limits as for pg_pan_gainloss.  The permutation step comes from the backend's pga_pan_phylosig.
 * sizeof(pg_phylosig_opt_t) is 40. */
typedef struct {
	int32_t type;        /* PG_DIST_GENE or PG_DIST_ADJ [gene] */
	int32_t metric;      /* PG_DIST_JACCARD or PG_DIST_DIFF [jaccard] */
	int32_t method;      /* PG_TREE_NJ or PG_TREE_UPGMA [upgma] */
	int32_t gain, loss;  /* the cost of a gain and of a loss, 1 .. 255 [1, 1] */
	int32_t n_perm;      /* permutations, 0 .. 2^31 - 2; 0: none [1000] */
	uint32_t seed;       /* of the permutations [11] */
	int32_t min_count;   /* an item is tested when it is present in >= min_count and absent from >= min_count assemblies; >= 1 [2] */
	double  max_p;       /* the table keeps the items with min(p_signal, p_scatter) <= max_p [1.0: all] */
} pg_phylosig_opt_t;
void pg_phylosig_opt_init(pg_phylosig_opt_t *o);
int  pg_phylosig_file(const char *gfa_fn, const pg_phylosig_opt_t *o);
void pg_write_phylosig(pg_graph_t *g, const pg_phylosig_opt_t *o);
int  pg_pan_phylosig(const uint8_t *presence, int32_t n_item, int32_t n_asm, const int64_t *rec, int32_t method, const pg_phylosig_opt_t *o, int32_t *out_i32,
                     int64_t *out_sum_i64);

/* Principal coordinates of the assemblies: classical scaling (cmdscale of R, pcoa of ape and scikit-bio) of one distance matrix, the
 * plot that shows the groups pg_cluster_* names and pg_permanova_* tests.  DESIGN.md section 8 "Principal coordinates" holds the
 * definition.  Input: a fixed-point matrix q over N assemblies, symmetric, zero diagonal, entries in [0, 2^29), F fraction bits,
 * d = q 2^-F.  A = -1/2 d o d entrywise, B = J A J with J = I - 11'/N, B = V L V'.  The axes are the n_axis ALGEBRAICALLY largest
 * eigenvalues l_1 >= ... (diff and plain Jaccard are not Euclidean: B then has negative eigenvalues, which are never axes); axis a is
 * reported when l_a > 1e-9 l_1, so fewer than n_axis axes may come back; an n_axis above N - 1 is N - 1.  Coordinates x_ia = v_ia
 * sqrt(l_a); sign: the component of v_a largest in size is positive, the first one on an exact tie (near-ties are decided by rounding:
 * compare after aligning the signs).  trace(B) = T / (2 N) 4^-F with T = the sum of q_ij^2 over i != j, an exact 128-bit sum converted
 * with one long double division; Explained = l_a / trace(B), whose denominator is the sum of ALL eigenvalues, the negative ones
 * included, so that it can overstate an axis' share for a metric that is not Euclidean.  The eigenpairs come from the backend's
 * pga_pan_pcoa: Lanczos with full reorthogonalisation, start vectors from the counter (seed, i); it stops when every wanted pair has a
 * residual <= 1e-10 l_1 or after 256 vectors (PANGENE_PCOA_STEPS lowers that for tests), and then says converged 0, prints the residuals
 * and leaves a note on stderr; that is no error.  Floating point: two builds agree within tolerances, not byte for byte; the same call
 * on the same build returns the same bits.
 * Output, tab-separated: one line "# items T / metric M / N / Fbits / trace / steps / restarts / converged" as name-value fields, then
 * "EV Axis Eigenvalue Explained Cumulative Residual" and one EV line per axis, then "PC Asm PC1 .. PCk" and one PC line per assembly;
 * numbers %.6g, Explained and Cumulative %.4f.  N < 3 or no distance above zero: the # line, a note on stderr and no table.
 * pg_pcoa_file: 0, -1 (the GFA file cannot be opened) or -2 (the backend's status is on stderr); pg_write_pcoa: the same for the graph
 * in memory; errors go to pg_last_error.
 * pg_pan_pcoa: any such matrix, int32 [n][n], with fbits fraction bits (PGA_ERR_ARG when it is not symmetric, has a diagonal entry that
 * is not zero or a negative entry, PGA_ERR_RANGE for an entry of 2^29 or more, for n > 16 384 and for an n_axis outside 1 .. 16); of the
 * options n_axis and seed are read.  Fills eig[n_axis], resid[n_axis], coord[n][n_axis] (row-major; the columns past the axes returned
 * are zero), trace and info[4] = axes returned, steps, converged, restarts, and returns 0 or a negative PGA_ERR_*.
 * pg_pan_pcoa_presence: the same for an item x assembly presence matrix [n_item][n_asm] and the distance `metric` of the options;
 * frac_bits receives F.  sizeof(pg_pcoa_opt_t) is 16. */
typedef struct {
	int32_t  type;    /* PG_DIST_GENE or PG_DIST_ADJ [gene] */
	int32_t  metric;  /* PG_DIST_JACCARD or PG_DIST_DIFF [jaccard] */
	int32_t  n_axis;  /* axes, 1 .. 16 [3] */
	uint32_t seed;    /* of the start vectors [0] */
} pg_pcoa_opt_t;
void pg_pcoa_opt_init(pg_pcoa_opt_t *o);
int  pg_pcoa_file(const char *gfa_fn, const pg_pcoa_opt_t *o);
void pg_write_pcoa(pg_graph_t *g, const pg_pcoa_opt_t *o);
int  pg_pan_pcoa(const int32_t *q, int32_t n, int32_t fbits, const pg_pcoa_opt_t *o, double *eig, double *resid, double *coord, double *trace, int32_t *info);
int  pg_pan_pcoa_presence(const uint8_t *presence, int32_t n_item, int32_t n_asm, const pg_pcoa_opt_t *o, double *eig, double *resid, double *coord, double *trace,
                          int32_t *info, int32_t *frac_bits);

/* Gene-trait tests adjusted for population structure: the Rao score test of every gene against a trait, with the principal coordinates
 * of pg_pcoa_* as covariates -- what a fixed-effects GWAS does with its principal components.  DESIGN.md section 8 "Structure-adjusted
 * association" holds the definition.  A screening test: one null fit per trait, one matrix product for all genes, no per-gene fit.
 * For a trait, N = the assemblies with a value and Z = [1, z_1 .. z_k] over them: the n_axis axes pcoa_core returns for ALL assemblies
 * (distance of `type` and `metric`, start vectors from `seed`), each divided by sqrt(eigenvalue / assemblies); fewer when fewer come
 * back, none for n_axis = 0.  Null model: PG_GLM_BINARY, logistic regression of y on Z by Newton steps from (logit mean(y), 0 ..),
 * the step halved up to 10 times while the log-likelihood falls, converged when the largest change of a coefficient is <= 1e-9, at
 * most 30 iterations; Fit 0 (a note, no gene lines) when the cap is reached, when any |eta_i| > 30 at convergence (separation) or when
 * the Cholesky factorisation fails; r = y - mu, w = mu (1 - mu).  PG_GLM_QUANT, least squares: s2 = RSS / (N - k - 1), r = (y - mu) / s2,
 * w = 1 / s2.  A trait with N < k + 3 or one value only is skipped with a note.  Per gene with presence x over the N assemblies:
 * a = sum x, U = x.r, s_w = x.w, b = (s_w, x.(w z_1) ..), V = s_w - |L^-1 b|^2 with L the Cholesky factor of Z'WZ.  A gene is eligible
 * when min(a, N - a) >= min_count, collinear when V <= 1e-8 s_w (printed with NA, left out of q and Lambda); otherwise Beta = U / V (the
 * exact least-squares coefficient for quant, the ONE-STEP estimate for binary), SE = 1 / sqrt(V), Z = U / sqrt(V), p = erfc(|Z| /
 * sqrt 2), q = Benjamini-Hochberg per trait over the tested genes, Lambda = median(Z^2) / 0.4549364 per trait.
 * Output, tab-separated, numbers %.6g: "# items / metric / A / Fbits / axes / family / converged" as name-value fields; "T Trait N
 * Cases|Mean Iter Fit Tested Collinear Lambda" and one T line per trait that was not skipped; "G Trait Gene N a Beta SE Z p q" and one G
 * line per eligible gene with p <= max_p (and per collinear one).  Floating point: two builds agree within tolerances, not byte for
 * byte; the same call on the same build returns the same bits.
 * pg_glm_file: 0, -1 (the GFA file cannot be opened), -2 (the backend's status is on stderr) or -3 (the trait file was turned down);
 * pg_write_glm: the same for the graph in memory; errors go to pg_last_error.
 * pg_pan_glm: any presence matrix uint8 [n_gene][n_asm], values double [n_trait][n_asm] (NaN = missing; 0 and 1 for PG_GLM_BINARY) and
 * explicit covariates double [n_asm][n_cov] (NULL with n_cov = 0), used as they are; of the options min_count is read.  Fills
 * out[n_trait][n_gene][4] = a, U, V, s_w (a = -1 and zeros for a gene that is not eligible or a trait without a fit) and
 * info[n_trait][4] = N, iterations, fit, tested, and returns 0 or a negative PGA_ERR_*: PGA_ERR_RANGE for n_cov > 13 or n_asm > 16 384,
 * PGA_ERR_ARG for an infinite value, a binary value that is not 0 or 1, or a covariate that is not finite.
 * sizeof(pg_glm_opt_t) is 32. */
#define PG_GLM_BINARY 0
#define PG_GLM_QUANT  1
typedef struct {
	int32_t  type;      /* of the distance: PG_DIST_GENE or PG_DIST_ADJ [gene] (the items tested are the genes) */
	int32_t  metric;    /* PG_DIST_JACCARD or PG_DIST_DIFF [jaccard] */
	int32_t  family;    /* PG_GLM_BINARY or PG_GLM_QUANT [binary] */
	int32_t  n_axis;    /* axes used as covariates, 0 .. 13; 0: intercept only [3] */
	uint32_t seed;      /* of the start vectors of the axes [0] */
	int32_t  min_count; /* a gene is tested when min(a, N - a) >= min_count [1] */
	double   max_p;     /* genes with p <= max_p are printed [1] */
} pg_glm_opt_t;
void pg_glm_opt_init(pg_glm_opt_t *o);
int  pg_glm_file(const char *gfa_fn, const char *trait_fn, const pg_glm_opt_t *o);
void pg_write_glm(pg_graph_t *g, const char *trait_fn, const pg_glm_opt_t *o);
int  pg_pan_glm(const uint8_t *presence, const double *values, int32_t n_gene, int32_t n_asm, int32_t n_trait, const double *covariates, int32_t n_cov, int32_t family,
                const pg_glm_opt_t *o, double *out, int32_t *info);

/* Gain and loss rates: `pangene rates`, `pangene --rates`.  The likelihood counterpart of pg_gainloss_*: a two-state Markov model
 * (gain rate lambda, 0 -> 1; loss rate mu, 1 -> 0) per item on the tree of the assemblies with its branch lengths, corrected for the
 * items nobody can observe, fitted by maximum likelihood.  DESIGN.md section 8 "Gain and loss rates" holds the definition.  Items and
 * tree are exactly those of pg_gainloss_* (type, metric, method); the branch lengths are those `pangene tree` prints (NJ's root sits in
 * the middle of the closing record's third branch), negative ones count as 0, and they are divided by their sum T and floored at 2^-20:
 * the rates are per item over the whole tree.  gain = loss = 0: the rates are fitted by a deterministic lattice search in
 * (log2 lambda, log2 mu); both > 0 (each in [1e-9, 1e9]): they are given and nothing is fitted; one without the other: PGA_ERR_ARG.
 * At the rates every item gets its log-likelihood lnL = ln L - ln(1 - L_absent), the posterior expected Gains and Losses -- the expected
 * numbers of branches with the item absent at the top and present at the bottom, and the reverse; NOT the expected numbers of events
 * along the branches, which are larger -- the posterior of the root, and a screening of nine rate multipliers r = 2^-4 .. 2^4: Rate =
 * the r with the largest lnL, LRT = 2 (lnL(Rate) - lnL(1)), p_rate = erfc(sqrt(LRT / 2)): the best of nine multipliers, not a maximum.
 * Output, tab-separated, numbers as %.6g.  The column header first, then one line "#" with items, metric, method, A, G (the items
 * used), gain, loss, lnL, rounds, converged and treelen (T in distance units) as NAME=VALUE fields.  out = PG_GAINLOSS_GENE:
 * "Gene Present lnL Gains Losses Changes Root Rate LRT p_rate", one line per item present somewhere with Changes = Gains + Losses >=
 * min_changes.  PG_GAINLOSS_NODE: "Node Child1 Child2 Leaves Length Present Gains Losses", the nodes named and ordered as
 * pg_gainloss_* does, Length normalised, the three sums over the items, NA for the root's Gains and Losses.  Fewer than two assemblies,
 * no items, or a tree without length: the header only, a note on stderr, status 0.
 * pg_rates_file: 0, -1 (the GFA file cannot be opened) or -2 (bad options, or the backend's status on stderr).  pg_write_rates: the same
 * for the graph in memory; errors go to pg_last_error.
 * pg_pan_rates: any presence matrix [n_item][n_asm] and any tree as records, as for pg_pan_gainloss, with the same refusals; of the
 * options gain and loss are read.  Fills fit_out[6] = lambda, mu, lnL, rounds, converged, T in record units; gene_out[n_item][7] = lnL,
 * gains, losses, root, rate, LRT, p_rate (NaN for an item absent from every assembly, which is left out of the fit and the totals);
 * node_out[2 n_asm - 1][4] = length (normalised), present, gains, losses in node id order.  Without a model (n_asm < 2, T = 0, no item
 * present anywhere) it returns 0 with NaN rates.  The likelihoods and posteriors come from the backend's pga_pan_rates.
 * sizeof(pg_rates_opt_t) is 40. */
typedef struct {
	int32_t type;        /* PG_DIST_GENE or PG_DIST_ADJ [gene] */
	int32_t metric;      /* PG_DIST_JACCARD or PG_DIST_DIFF [jaccard] */
	int32_t method;      /* PG_TREE_UPGMA or PG_TREE_NJ [upgma] */
	int32_t out;         /* PG_GAINLOSS_GENE or PG_GAINLOSS_NODE [gene] */
	double gain, loss;   /* the rates, both given or both 0 = fitted [0, 0] */
	double min_changes;  /* the gene table keeps the items with Changes >= min_changes [0: all] */
} pg_rates_opt_t;
void pg_rates_opt_init(pg_rates_opt_t *o);
int  pg_rates_file(const char *gfa_fn, const pg_rates_opt_t *o);
void pg_write_rates(pg_graph_t *g, const pg_rates_opt_t *o);
int  pg_pan_rates(const uint8_t *presence, int32_t n_item, int32_t n_asm, const int64_t *rec, int32_t method, const pg_rates_opt_t *o, double *fit_out, double *gene_out,
                  double *node_out);

/* Last error of the path (0 = none).  The reference aborts on invariant violations; this library
 * records a status instead, prints one line to stderr, and leaves the graph empty. */
int         pg_last_error(void);
const char *pg_last_error_str(void);

/* Redirect what the writers would print to stdout into a file descriptor-less sink:
 * pg_set_output(path) makes pg_write_* append to `path` (NULL restores stdout). */
int pg_set_output(const char *path);

/* Register the gene/protein names (and lengths) of a PAF whose hits belong to ANOTHER shard, so that
 * first-seen id numbering (read.c:151-168) is identical on every rank.  Adds an empty genome. */
int32_t pg_scan_paf_ids(const pg_opt_t *opt, pg_data_t *d, const char *fn);

/* Parse n PAFs on host threads (n_threads <= 0: as many as the process may really use -- the affinity mask capped by the control
 * group's CPU quota -- and at most 64) and append them in the given order; gene / protein / contig ids and every attribute of every
 * gene and protein come out exactly as after n sequential pg_read_paf calls (tests/test_reader.py).  The hit / exon arrays of plain
 * (not gzipped) files lie in one huge-page mapping owned by `d`: pg_data_destroy releases it, nobody else may free() them.  ids_only (may be NULL): per file, non-zero = register
 * the names only, as pg_scan_paf_ids does.  Returns minus the number of files that could not be opened. */
int32_t pg_read_paf_batch(const pg_opt_t *opt, pg_data_t *d, int32_t n, const char *const *fns, const uint8_t *ids_only, int32_t n_threads);

/* Exchange hook: genomes shard across processes (one per GPU); the only communication is a handful
 * of small integer reductions / gathers per round.  NULL (default) = single process. */
enum { PG_X_I32 = 0, PG_X_I64 = 1 };
enum { PG_X_SUM = 0, PG_X_MAX = 1 };
typedef struct {
	int32_t rank, world;
	void *user;
	/* in-place all-reduce of `count` elements; is_device: buf is HBM (use RCCL) else host memory */
	int (*allreduce)(void *user, void *buf, int64_t count, int32_t dtype, int32_t op, int32_t is_device);
	/* all-gather `nbytes` from every rank into out[world*nbytes] */
	int (*allgather)(void *user, const void *in, void *out, int64_t nbytes, int32_t is_device);
	/* non-zero: the callbacks enqueue on the backend's own stream (pga_active_stream), so the library need not wait for
	 * its kernels before calling them; zero: it synchronises first */
	int32_t stream_ordered;
} pg_exchange_t;
void pg_set_exchange(const pg_exchange_t *x);

/* Built-in exchange for the HIP backend: RCCL collectives enqueued on the kernels' own stream (no host round trip).
 * Rank 0 obtains the 128-byte bootstrap id, the launcher hands it to every rank, every rank calls pg_rccl_init with
 * its HIP device current; this installs the exchange (pg_set_exchange).  0 on success; pg_rccl_error() says why not. */
int pg_rccl_unique_id(void *out128);
int pg_rccl_init(int32_t rank, int32_t world, const void *id128);
int pg_rccl_finalize(void);
const char *pg_rccl_error(void);

/* The exchange between the processes one command forks, for backends whose vectors live in host memory (the HIP backend uses
 * RCCL): the launcher maps a shared region before the fork (pg_shm_create), every rank installs it after (pg_shm_init). */
void *pg_shm_create(int32_t world, int64_t slot_bytes);
int pg_shm_init(void *region, int32_t rank);
/* 1 when the linked backend keeps its vectors in device memory (HIP), 0 otherwise; the HIP device a process is to use */
int pg_backend_is_device(void);
int pg_set_device(int32_t device);
int pg_device_count(void);

/* Wall-clock seconds spent inside the last pg_post_process + pg_graph_gen (stages A+B+C), and the
 * number of hits they processed (local shard). */
double  pg_last_path_seconds(void);
int64_t pg_last_path_hits(void);
/* how many times the last pg_graph_gen ran stages A-C: 1, plus one for every repeat after a tie-order hazard on a contig that did
 * not follow the reference's exact order yet (mode auto; DESIGN.md "bit-identity") */
int     pg_last_attempts(void);
double  pg_last_upload_seconds(void);   /* allocation + H2D copy + order-replay set-up of the last pg_post_process (0 for a resident rerun) */
double  pg_last_pack_seconds(void);     /* wall seconds the reader spent packing the genomes of the last upload into their blocks */
/* hits and exons of the local shard of d (what the last pg_post_process uploaded) */
int     pg_shard_counts(const pg_data_t *d, int64_t *n_hit, int64_t *n_exon);

/* pg_post_process / pg_graph_gen leave the per-hit FLAG fields of the host records (flt, shadow, rank, ...) on the
 * device until a writer needs them: pg_write_graph/pg_write_walk only fetch one flt bit per hit, pg_write_bed
 * fetches everything.  A caller that reads d->genome[j].hit[i] itself calls this first.
 * The same holds for what pg_post_process computes per protein and per gene -- d->prot[i].n / avg_score_adj /
 * max_score_ori / rep and d->gene[i].rep_pid: between pg_post_process and the end of pg_graph_gen they may still hold
 * the previous pass's values (or zeros); they are current after pg_graph_gen, after any writer, and after this call. */
int pg_sync_host(pg_data_t *d);

/* Tie-order policy (see DESIGN.md "bit-identity"): 0 canonical stable order everywhere; 1 (default,
 * env PANGENE_EXACT=auto) replay the reference's unstable sort for the first contig of genomes whose
 * leading tie group has >= 2 hits; 2 (PANGENE_EXACT=all) replay it for every contig. */
void pg_set_exact_mode(int mode);

/* Benchmark support: make the next pg_post_process(opt, d) restart stages A+B+C on the shard that is
 * already resident in HBM (no re-pack, no PCIe upload).  The host hit arrays are left as they are. */
int pg_rerun_resident(pg_data_t *d);

/* HIP-event timing of kernel classes of the runs since the last pg_kernel_timing_reset (which also switches the
 * timing on): which 0 = stage-A sweep pg_shadow(cal_dom_sc=1) ("K1", the hit-filter+overlap kernel), 1 = pg_flt_ov_isoform
 * sweep, 2 = (not timed any more: the stage-C sweeps), 3 = all of stage A (sorts, per-hit constants, pg_flag_pseudo, sweeps, filters),
 * 4 = no kernel class: n_launch = the number of times the host waited for the backend's stream since the reset; 5 / 6 (with PANGENE_TIME_ROUNDS=1 at
 * the reset) = every pg_gen_arc round / its walk alone, which | (k + 1) << 8 = the k-th timed launch of the class alone; 7 = no timing: which
 * build of K1 the upload got (n_launch 1 = exon lists staged in LDS, 0 = read in place, -1 = not decided), total_ms = the sampled exons a tile. */
int pg_kernel_timing(pg_data_t *d, int32_t which, double *total_ms, int64_t *n_launch, int64_t *units);
double pg_last_reserve_seconds(void); /* what the last pg_read_paf_batch spent reserving device memory before it parsed (large data sets: pga_reserve) */
int pg_kernel_timing_reset(pg_data_t *d);
/* collectives the driver has issued through the exchange callbacks so far, in this process (bench.py: per pass of a sharded run) */
int64_t pg_collective_count(void);

/* Page-locked host memory: the library keeps the pinned slabs of an upload for the next one (up to 4 GiB while a data set is
 * alive; 256 MiB after the last pg_data_destroy).  A long-lived host calls this to give back what exceeds keep_bytes (0 = all). */
void pg_trim_host_cache(size_t keep_bytes);

/* Bring the device runtime up and load the library's kernels ahead of the first pg_post_process (a command line calls it on a
 * helper thread while the PAF files are parsed); a no-op on backends without a device */
int pg_device_warm(void);

/* HBM bandwidth a plain copy kernel reaches on the current device, GB/s of read + write (measurement support: the calibration
 * SURVEY.md 8d asks for beside the spec peak); negative without a device */
double pg_device_copy_gbps(size_t bytes, int32_t reps);

/* wall seconds the host driver spent per phase of the last run (names via pg_phase_name) */
int pg_phase_times(double *out, int n);
const char *pg_phase_name(int i);

#ifdef __cplusplus
}
#endif
#endif
