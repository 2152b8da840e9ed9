// pangene command line: `pangene [options] <in.paf> [...] > graph.gfa` with the reference's option
// letters, defaults and usage text (main.c:12-152, option.c:9-25), on top of libpangene_amd.
#include <dlfcn.h>
#include <getopt.h>
#include <signal.h>
#include <sys/prctl.h>
#include <sys/resource.h>
#include <sys/stat.h>
#include <sys/wait.h>
#include <unistd.h>
#include <cctype>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <string>
#include <thread>
#include <vector>
#include "pangene_amd.h"

static int usage(FILE *fp, const pg_opt_t *opt)
{
	std::fprintf(fp, "Usage: pangene [options] <in.paf> [...]\n");
	std::fprintf(fp, "Options:\n");
	std::fprintf(fp, "  Input preprocessing:\n");
	std::fprintf(fp, "    -d CHAR       gene-protein delimiter [%c]\n", opt->gene_delim);
	std::fprintf(fp, "    -X STR/@FILE  exclude genes in STR list or in @FILE []\n");
	std::fprintf(fp, "    -I STR/@FILE  include genes in the output graph []\n");
	std::fprintf(fp, "    -P STR/@FILE  prioritize genes in the output graph []\n");
	std::fprintf(fp, "    -e FLOAT      drop an alignment if its identity <FLOAT [%g]\n", opt->min_prot_iden);
	std::fprintf(fp, "    -l FLOAT      drop an alignment if <FLOAT fraction of the protein aligned [%g]\n", opt->min_prot_ratio);
	std::fprintf(fp, "    -m FLOAT      score adjustment coefficient [%g]\n", opt->score_adj_coef);
	std::fprintf(fp, "  Graph construction:\n");
	std::fprintf(fp, "    -f FLOAT      min overlap fraction [%g]\n", opt->min_ov_ratio);
	std::fprintf(fp, "    -J            don't filter pseudogenes across samples\n");
	std::fprintf(fp, "    -E            ignore genes that are single-exon in all genomes\n");
	std::fprintf(fp, "    -p FLOAT      gene considered if dominant in FLOAT fraction of genes [%g]\n", opt->min_vertex_ratio);
	std::fprintf(fp, "    -c INT        drop a gene if average occurrence is >INT [%d]\n", opt->max_avg_occ);
	std::fprintf(fp, "    -g INT        drop a gene if its in- or out-degree >INT [%d]\n", opt->max_degree);
	std::fprintf(fp, "    -r INT        drop a gene if it connects >INT distant loci [%d]\n", opt->max_dist_loci);
	std::fprintf(fp, "    -b FLOAT      demote a branching arc if weaker than the best by FLOAT [%g]\n", opt->branch_diff);
	std::fprintf(fp, "    -B FLOAT      cut a branching arc if weaker by FLOAT [%g]\n", opt->branch_diff_cut);
	std::fprintf(fp, "    -y FLOAT      cut a distant branching arc if weaker by FLOAT [%g]\n", opt->branch_diff_dist);
	std::fprintf(fp, "    -T INT        apply branch cutting for INT times [%d]\n", opt->n_branch_flt);
	std::fprintf(fp, "    -F            don't consider genes on different contigs as distant\n");
	std::fprintf(fp, "    -a INT        prune an arc if it is supported by <INT genomes [%d]\n", opt->min_arc_cnt);
	std::fprintf(fp, "  Output:\n");
	std::fprintf(fp, "    -w            Suppress walk lines (W-lines)\n");
	std::fprintf(fp, "    --bed[=STR]   output 12-column BED where STR is walk, raw or flag [walk]\n");
	std::fprintf(fp, "    --matrix[=STR] output the gene x assembly matrix of pangene.js gfa2matrix, STR presence or count [presence]\n");
	std::fprintf(fp, "    --gpus=INT    shard the genomes over INT GPUs of this node: one process per device, RCCL over xGMI [1]\n");
	std::fprintf(fp, "    --version     print version number\n");
	std::fprintf(fp, "    --call        output the bubbles and alleles of pangene.js call (default options) instead of the graph\n");
	std::fprintf(fp, "    --curves[=INT] output pan/core/new/unique accumulation curves over INT orders of the assemblies [10]\n");
	std::fprintf(fp, "    --curves-seed=INT  seed of the orders of --curves [11]\n");
	std::fprintf(fp, "    --dist[=STR]  output pairwise distances of the assemblies over gene content (gene) or gene adjacencies (adj) [gene]\n");
	std::fprintf(fp, "    --dist-metric=STR  metric of --dist: jaccard, shared or diff [jaccard]\n");
	std::fprintf(fp, "    --assoc[=FLOAT] output the gene pairs whose presence over the assemblies is correlated, |phi| >= FLOAT [0.8]\n");
	std::fprintf(fp, "    --assoc-min-count=INT  --assoc: a gene takes part when it is present in >=INT and absent from >=INT assemblies [2]\n");
	std::fprintf(fp, "    --assoc-sign=STR  --assoc: keep pos (co-occurring), neg (avoiding) or both [both]\n");
	std::fprintf(fp, "    --trait=FILE  output the association of every gene with the binary traits of FILE (assembly, then 1/0/NA per trait)\n");
	std::fprintf(fp, "    --trait-perm=INT  --trait: label permutations [1000]\n");
	std::fprintf(fp, "    --trait-seed=INT  --trait: seed of the permutations [11]\n");
	std::fprintf(fp, "    --trait-lineage=STR  --trait: add the pairwise comparisons on the nj or upgma tree of the assemblies (pairs supp opp p_pair_best p_pair_worst)\n");
	std::fprintf(fp, "    --qtrait=FILE  output the rank-sum association of every gene with the quantitative traits of FILE (assembly, then a number or NA per trait)\n");
	std::fprintf(fp, "    --qtrait-perm=INT  --qtrait: permutations of the values [1000]\n");
	std::fprintf(fp, "    --qtrait-seed=INT  --qtrait: seed of the permutations [11]\n");
	std::fprintf(fp, "    --tree[=STR]  output a tree of the assemblies (Newick) from their gene (gene) or gene-adjacency (adj) distances [gene]\n");
	std::fprintf(fp, "    --tree-metric=STR  distance of --tree: jaccard or diff [jaccard]\n");
	std::fprintf(fp, "    --tree-method=STR  --tree: nj (neighbour-joining, unrooted; negative branch lengths are printed as they come) or upgma [nj]\n");
	std::fprintf(fp, "    --tree-boot=INT    --tree: bootstrap replicates over the items; inner nodes are labelled with their support in per cent [0]\n");
	std::fprintf(fp, "    --tree-seed=INT    seed of the bootstrap draws [0]\n");
	std::fprintf(fp, "    --cluster=INT[-INT]  output k-medoids clusters of the assemblies for k = INT, or for every k of the range and the assignment of the best one\n");
	std::fprintf(fp, "    --cluster-type=STR   --cluster: items, gene or adj [gene]\n");
	std::fprintf(fp, "    --cluster-metric=STR --cluster: distance, jaccard or diff [jaccard]\n");
	std::fprintf(fp, "    --cluster-iter=INT   --cluster: swap iterations per k at the most [1000]\n");
	std::fprintf(fp, "    --permanova=FILE  output the two-group PERMANOVA of the assemblies' distances for the binary traits of FILE (pseudo-F, R2, permutation p)\n");
	std::fprintf(fp, "    --permanova-type=STR    --permanova: items, gene or adj [gene]\n");
	std::fprintf(fp, "    --permanova-metric=STR  --permanova: distance, jaccard or diff [jaccard]\n");
	std::fprintf(fp, "    --permanova-perm=INT    --permanova: label permutations [1000]\n");
	std::fprintf(fp, "    --permanova-seed=INT    --permanova: seed of the permutations [11]\n");
	std::fprintf(fp, "    --mantel[=FILE]   output the Mantel test of two distance matrices of the assemblies, or of one and the matrix of FILE (r, permutation p)\n");
	std::fprintf(fp, "    --mantel-x=STR    --mantel: the first matrix, gene|adj:jaccard|diff [gene:jaccard]\n");
	std::fprintf(fp, "    --mantel-y=STR    --mantel: the second matrix, unless FILE is given [adj:jaccard]\n");
	std::fprintf(fp, "    --mantel-perm=INT --mantel: permutations of the assemblies [1000]\n");
	std::fprintf(fp, "    --mantel-seed=INT --mantel: seed of the permutations [11]\n");
	std::fprintf(fp, "    --gainloss[=STR]  output the gains and losses of every item on the tree of the assemblies, per item (gene) or per branch (node) [gene]\n");
	std::fprintf(fp, "    --gainloss-type=STR     --gainloss: items, gene or adj [gene]\n");
	std::fprintf(fp, "    --gainloss-metric=STR   --gainloss: distance of the tree, jaccard or diff [jaccard]\n");
	std::fprintf(fp, "    --gainloss-method=STR   --gainloss: upgma, or nj rooted at its closing join ((x, y), z): gains and losses depend on that reading [upgma]\n");
	std::fprintf(fp, "    --gainloss-gain=INT     --gainloss: cost of a gain, 1 to 255 [1]\n");
	std::fprintf(fp, "    --gainloss-loss=INT     --gainloss: cost of a loss, 1 to 255 [1]\n");
	std::fprintf(fp, "    --gainloss-resolve=STR  --gainloss: on a tie a change sits towards the tips (late) or towards the root (early) [late]\n");
	std::fprintf(fp, "    --gainloss-min=INT      --gainloss=gene: print the items with at least INT changes [0]\n");
	std::fprintf(fp, "    --coevo[=FLOAT]   output the item pairs gained and lost on the same branches of the tree of the assemblies with |r| >= FLOAT [0.8]\n");
	std::fprintf(fp, "    --coevo-type=STR        --coevo: items, gene or adj [gene]\n");
	std::fprintf(fp, "    --coevo-metric=STR      --coevo: distance of the tree, jaccard or diff [jaccard]\n");
	std::fprintf(fp, "    --coevo-method=STR      --coevo: upgma, or nj rooted at its closing join ((x, y), z): the events depend on that reading [upgma]\n");
	std::fprintf(fp, "    --coevo-gain=INT        --coevo: cost of a gain, 1 to 255 [1]\n");
	std::fprintf(fp, "    --coevo-loss=INT        --coevo: cost of a loss, 1 to 255 [1]\n");
	std::fprintf(fp, "    --coevo-resolve=STR     --coevo: on a tie a change sits towards the tips (late) or towards the root (early) [late]\n");
	std::fprintf(fp, "    --coevo-min=INT         --coevo: an item takes part with at least INT events; with 1 every pair of strain-specific genes of one assembly scores 1 [2]\n");
	std::fprintf(fp, "    --coevo-sign=STR        --coevo: keep pos, neg or both [both]\n");
	std::fprintf(fp, "    --coevo-max=INT         --coevo: give up when more than INT pairs pass [16777216]\n");
	std::fprintf(fp, "  Also: pangene gfa2matrix [-c] [-d FILE] [-p] <in.gfa>   (pangene.js gfa2matrix on a GFA file)\n");
	std::fprintf(fp, "        pangene call [-m INT] [-w] [-b] [-e] [-d] [-p] [-s] [-r STR] <in.gfa>   (pangene.js call on a GFA file)\n");
	std::fprintf(fp, "        pangene curves [-n INT] [-s INT] <in.gfa>   (accumulation curves of the gfa2matrix matrix of a GFA file)\n");
	std::fprintf(fp, "        pangene dist [-t gene|adj] [-m jaccard|shared|diff] [-p] <in.gfa>   (pairwise distances of the assemblies of a GFA file)\n");
	std::fprintf(fp, "        pangene assoc [-r FLOAT] [-c INT] [-s pos|neg|both] [-x INT] <in.gfa>   (co-occurring and avoiding gene pairs of a GFA file)\n");
	std::fprintf(fp, "        pangene trait -t FILE [-n INT] [-s INT] [-c INT] [-p FLOAT] <in.gfa>   (gene-trait association over the matrix of a GFA file; -L nj|upgma adds the lineage-aware pairwise comparisons)\n");
	std::fprintf(fp, "        pangene qtrait -t FILE [-n INT] [-s INT] [-c INT] [-p FLOAT] <in.gfa>   (rank-sum test of every gene against the quantitative traits of a trait file)\n");
	std::fprintf(fp, "        pangene tree [-t gene|adj] [-m jaccard|diff] [-a nj|upgma] [-b INT] [-s INT] <in.gfa>   (neighbour-joining or UPGMA tree of the assemblies of a GFA file, with bootstrap support)\n");
	std::fprintf(fp, "        pangene cluster [-t gene|adj] [-m jaccard|diff] -k INT[-INT] [-i INT] <in.gfa>   (k-medoids clusters of the assemblies of a GFA file, their medoids and silhouettes)\n");
	std::fprintf(fp, "        pangene permanova -t FILE [-T gene|adj] [-m jaccard|diff] [-n INT] [-s INT] <in.gfa>   (do the two groups of a binary trait differ in gene content: pseudo-F, R2 and a permutation p per trait)\n");
	std::fprintf(fp, "        pangene mantel [-x SPEC] [-y SPEC | -f FILE] [-n INT] [-s INT] <in.gfa>   (do two distance matrices of the assemblies agree: Mantel's r and its permutation p)\n");
	std::fprintf(fp, "        pangene gainloss [-t gene|adj] [-m jaccard|diff] [-a upgma|nj] [-g INT] [-l INT] [-r late|early] [-o gene|node] [-c INT] <in.gfa>   (gene gains and losses on the tree of the assemblies by parsimony, per item or per branch)\n");
	std::fprintf(fp, "        pangene coevo [-t gene|adj] [-m jaccard|diff] [-a upgma|nj] [-g INT] [-l INT] [-e late|early] [-r FLOAT] [-c INT] [-s pos|neg|both] [-x INT] <in.gfa>   (item pairs gained and lost on the same branches of the tree of the assemblies)\n");
	return fp == stdout ? 0 : 1;
}

static int64_t parse_num(const char *s) // "2m", "500k", ... (main.c:45-55)
{
	char *p;
	double x = std::strtod(s, &p);
	if (*p == 'G' || *p == 'g') x *= 1e9;
	else if (*p == 'M' || *p == 'm') x *= 1e6;
	else if (*p == 'K' || *p == 'k') x *= 1e3;
	return (int64_t)(x + .499);
}

static int main_gfa2matrix(int argc, char *argv[]) // pangene.js:1168-1183
{
	int c, copy_number = 0, print_cd = 0;
	const char *clstr = nullptr;
	while ((c = getopt(argc, argv, "cd:p")) >= 0) {
		if (c == 'c') copy_number = 1;
		else if (c == 'd') clstr = optarg;
		else if (c == 'p') print_cd = 1;
	}
	if (argc - optind < 1) {
		std::puts("Usage: pangene gfa2matrix [options] <in.gfa>\nOptions:\n  -c        output counts\n  -d FILE   CD-HIT cluster file to merge paralogs []");
		return 0;
	}
	return pg_gfa2matrix_file(argv[optind], copy_number, clstr, print_cd) == 0 ? 0 : 1;
}

// `pangene call` = pangene.js call (pangene.js:941-980): bubbles of a GFA and the alleles its walks take through them
static int32_t js_int(const char *s) // parseInt; its NaN behaves like a limit nothing exceeds
{
	while (*s && std::isspace((unsigned char)*s)) ++s;
	const char *p = s + (*s == '+' || *s == '-');
	if (*p < '0' || *p > '9') return INT32_MAX;
	const double x = std::strtod(std::string(s, (size_t)(p - s) + std::strspn(p, "0123456789")).c_str(), nullptr);
	return x > INT32_MAX ? INT32_MAX : x < INT32_MIN ? INT32_MIN : (int32_t)x;
}

static int main_call(int argc, char *argv[])
{
	pg_call_opt_t o;
	pg_call_opt_init(&o);
	int c;
	while ((c = getopt(argc, argv, "bedpm:wr:s")) >= 0) {
		if (c == 'b') o.print_bandage = 1;
		else if (c == 'e') o.print_cec = 1;
		else if (c == 'd') o.print_dfs = 1;
		else if (c == 'm') o.max_ext = js_int(optarg);
		else if (c == 'w') o.ignore_walk = 1;
		else if (c == 'r') o.ref = optarg;
		else if (c == 'p') o.use_pst = 1;
		else if (c == 's') o.add_super = 1;
	}
	if (argc - optind < 1) {
		std::printf("Usage: pangene call [options] <in.gfa>\nOptions:\n  General:\n    -m INT   don't output gene lists longer than INT [%d]\n"
		            "    -w       ignore walks\n    -b       output equivalent classes for Bandage visualization\n  Use PST:\n"
		            "    -p       use program structure tree (PST) to find bubbles\n"
		            "    -s       add a super node (preferred and only effectively with -p)\n"
		            "    -r INT   reference assembly for additional edges to the super node []\n"
		            "  Debugging:\n    -d       output DFS traversal\n    -e       output cycle equivalent class\n", o.max_ext);
		return 0;
	}
	return pg_call_file(argv[optind], &o) == 0 ? 0 : 1;
}

// ---------------------------------------------------------------------------------------------------------------
// The analyses: `pangene NAME [options] <in.gfa>` on a GFA file and `pangene --NAME[=X] --NAME-sub=X <in.paf> [...]` on the graph in
// memory.  Both spellings, their refusals and the dispatch come from ONE table, kAnalyses below: a record per analysis, a row per option.
// ---------------------------------------------------------------------------------------------------------------
union AnyOpt { pg_curves_opt_t curves; pg_dist_opt_t dist; pg_assoc_opt_t assoc; pg_trait_opt_t trait; pg_tree_opt_t tree; pg_qtrait_opt_t qtrait;
	pg_cluster_opt_t cluster; pg_permanova_opt_t permanova; pg_mantel_opt_t mantel; pg_gainloss_opt_t gainloss; pg_coevo_opt_t coevo; pg_phylosig_opt_t phylosig; pg_pcoa_opt_t pcoa; pg_glm_opt_t glm; pg_rates_opt_t rates; };

struct Word { const char *s; int32_t v; };
static const Word W_TYPE[] = { { "gene", PG_DIST_GENE }, { "adj", PG_DIST_ADJ }, { nullptr, 0 } };
static const Word W_DIST_METRIC[] = { { "jaccard", PG_DIST_JACCARD }, { "shared", PG_DIST_SHARED }, { "diff", PG_DIST_DIFF }, { nullptr, 0 } };
static const Word W_METRIC[] = { { "jaccard", PG_DIST_JACCARD }, { "diff", PG_DIST_DIFF }, { nullptr, 0 } };
static const Word W_METHOD[] = { { "nj", PG_TREE_NJ }, { "upgma", PG_TREE_UPGMA }, { nullptr, 0 } };
static const Word W_SIGN[] = { { "both", PG_ASSOC_BOTH }, { "pos", PG_ASSOC_POS }, { "neg", PG_ASSOC_NEG }, { nullptr, 0 } };
static const Word W_LINEAGE[] = { { "nj", PG_LINEAGE_NJ }, { "upgma", PG_LINEAGE_UPGMA }, { nullptr, 0 } };
static const Word W_MODE[] = { { "late", PG_GAINLOSS_LATE }, { "early", PG_GAINLOSS_EARLY }, { nullptr, 0 } };
static const Word W_OUT[] = { { "gene", PG_GAINLOSS_GENE }, { "node", PG_GAINLOSS_NODE }, { nullptr, 0 } };
static const Word W_FAMILY[] = { { "binary", PG_GLM_BINARY }, { "quant", PG_GLM_QUANT }, { nullptr, 0 } };

struct Row;
typedef bool (*Reader)(const char *s, void *field, const Row &r); // false: not a value of this option
struct Row {
	char letter;          // of the subcommand (0: none)
	const char *suffix;   // --NAME-suffix (nullptr: none)
	Reader read;          // (nullptr ends the rows of an analysis)
	size_t field;         // offset in the analysis' pg_NAME_opt_t
	long long lo, hi;     // integer readers: the bounds
	const Word *words;    // rd_word: the list
	const char *msg;      // "ERROR: -x <msg>" / "ERROR: --NAME-suffix <msg>"
	bool extra = false;   // --NAME-suffix without --NAME is refused
	const char *long_msg = nullptr; // where --NAME says something else than the letter does
	bool no_file = false; // cannot be combined with the side file
	bool late = false;    // subcommand, rd_atoi rows (int32 fields) only: lo is checked after the last option, so that a later value mends an earlier one
};

static int word_of(const Word *w, const char *s) { for (; w->s; ++w) if (std::strcmp(w->s, s) == 0) return w->v; return -1; }
static bool strict_ll(const char *s, long long lo, long long hi, long long &x) // a whole number in [lo, hi] and nothing after it
{
	char *e = nullptr;
	x = std::strtoll(s, &e, 10);
	return e != s && *e == 0 && x >= lo && x <= hi;
}
static bool strict_real(const char *s, double &x) { char *e; x = std::strtod(s, &e); return e != s && *e == 0; }

static bool rd_i32(const char *s, void *f, const Row &r) { long long x; if (!strict_ll(s, r.lo, r.hi, x)) return false; *(int32_t *)f = (int32_t)x; return true; }
static bool rd_i64(const char *s, void *f, const Row &r) { long long x; if (!strict_ll(s, r.lo, r.hi, x)) return false; *(int64_t *)f = x; return true; }
static bool rd_u32(const char *s, void *f, const Row &) // a whole number that fits 32 bits; digits only (strtoull alone would take "-1" and " 7")
{
	char *end = nullptr;
	if (*s < '0' || *s > '9') return false;
	const unsigned long long x = std::strtoull(s, &end, 10);
	if (*end != 0 || end - s > 10 || x > 4294967295ull) return false;
	*(uint32_t *)f = (uint32_t)x;
	return true;
}
// the lax readers of the older options: whatever atoi / atoll / strtoul make of the text ("x" is 0, "3x" is 3)
static bool rd_atoi(const char *s, void *f, const Row &r) { return (*(int32_t *)f = std::atoi(s)) >= r.lo; }
static bool rd_atoll(const char *s, void *f, const Row &r) { return (*(int64_t *)f = std::atoll(s)) >= r.lo; }
static bool rd_strtoul(const char *s, void *f, const Row &) { *(uint32_t *)f = (uint32_t)std::strtoul(s, nullptr, 10); return true; }
static bool rd_unit(const char *s, void *f, const Row &) { double &x = *(double *)f; return strict_real(s, x) && x >= 0.0 && x <= 1.0; } // a number in [0, 1]
static bool rd_nonneg(const char *s, void *f, const Row &) { double &x = *(double *)f; return strict_real(s, x) && x >= 0.0; }
static bool rd_rate(const char *s, void *f, const Row &) { double &x = *(double *)f; return strict_real(s, x) && x >= 1e-9 && x <= 1e9; } // a rate (a NaN fails both tests)
static bool rd_word(const char *s, void *f, const Row &r) { return (*(int32_t *)f = word_of(r.words, s)) >= 0; }
static bool rd_flag(const char *, void *f, const Row &) { *(int32_t *)f = 1; return true; } // (an option without a value)
// "INT" or "INT-INT": a k or a range of k, 2 <= lo <= hi; digits only.  Fills the field (k_lo) and the one after it (k_hi).
static_assert(offsetof(pg_cluster_opt_t, k_hi) == offsetof(pg_cluster_opt_t, k_lo) + sizeof(int32_t), "rd_cluster_range fills k_lo and the int32 after it");
static bool rd_cluster_range(const char *s, void *f, const Row &)
{
	char *end = nullptr;
	if (*s < '0' || *s > '9') return false;
	const long long a = std::strtoll(s, &end, 10);
	long long b = a;
	if (*end == '-') {
		const char *t = end + 1;
		if (*t < '0' || *t > '9') return false;
		b = std::strtoll(t, &end, 10);
	}
	if (*end != 0 || a < 2 || b < a || b > 2147483647ll) return false;
	((int32_t *)f)[0] = (int32_t)a, ((int32_t *)f)[1] = (int32_t)b;
	return true;
}
// SPEC of mantel: gene|adj + ':' + jaccard|diff.  Fills the field (the type) and the one after it (the metric).
static_assert(offsetof(pg_mantel_opt_t, x_metric) == offsetof(pg_mantel_opt_t, x_type) + sizeof(int32_t) &&
              offsetof(pg_mantel_opt_t, y_metric) == offsetof(pg_mantel_opt_t, y_type) + sizeof(int32_t), "rd_mantel_spec fills a type and the int32 after it");
static bool rd_mantel_spec(const char *s, void *f, const Row &)
{
	const char *c = std::strchr(s, ':');
	if (c == nullptr) return false;
	const int ty = word_of(W_TYPE, std::string(s, c).c_str()), me = word_of(W_METRIC, c + 1);
	if (ty < 0 || me < 0) return false;
	((int32_t *)f)[0] = ty, ((int32_t *)f)[1] = me;
	return true;
}

// the rows by what reads them
static constexpr long long INT31 = 2147483647ll;
static constexpr Row word(char l, const char *suf, size_t f, const Word *w, const char *msg, bool extra = false) { return { l, suf, rd_word, f, 0, 0, w, msg, extra }; }
static constexpr Row i32(char l, const char *suf, size_t f, long long lo, long long hi, const char *msg, bool extra = false) { return { l, suf, rd_i32, f, lo, hi, nullptr, msg, extra }; }
static constexpr Row plain(char l, const char *suf, Reader rd, size_t f, const char *msg, bool extra = false, long long lo = 0) { return { l, suf, rd, f, lo, 0, nullptr, msg, extra }; }
static constexpr Row seed(char l, size_t f, bool extra = false) { return plain(l, "seed", rd_strtoul, f, "", extra); } // (never refused)
static constexpr Row i64(char l, const char *suf, size_t f, long long lo, long long hi, const char *msg, bool extra = false) { return { l, suf, rd_i64, f, lo, hi, nullptr, msg, extra }; }
// a lax count of the subcommand alone, at least lo, checked late (Row::late); --NAME=X reads it too, checks at once and says long_msg
static constexpr Row late_count(char l, size_t f, long long lo, const char *msg, const char *long_msg)
{
	Row r = plain(l, nullptr, rd_atoi, f, msg, false, lo);
	r.long_msg = long_msg, r.late = true;
	return r;
}
static constexpr Row spec(char l, const char *suf, size_t f, bool no_file) { return { l, suf, rd_mantel_spec, f, 0, 0, nullptr, "must be gene|adj:jaccard|diff", true, nullptr, no_file }; }
static constexpr const char *M_TYPE = "must be gene or adj";
static constexpr const char *M_METRIC = "must be jaccard or diff (shared is not a distance)";
static constexpr const char *M_PERM = "must be in [0, 2147483646]";
static constexpr const char *M_INT31 = "must be in [0, 2147483647]";
static constexpr const char *M_COST = "must be in [1, 255]";
static constexpr const char *M_UNIT = "must be in [0, 1]";
static constexpr const char *M_MIN1 = "must be at least 1";
static constexpr const char *M_NONNEG = "must not be negative";
static constexpr const char *M_SIGN = "must be pos, neg or both";
static constexpr const char *M_MODE = "must be late or early";

// pg_NAME_opt_init, pg_NAME_file and pg_write_NAME behind one signature; `side` is the trait or matrix file of the analyses that take one
struct Calls {
	void (*init)(AnyOpt *o);
	int (*file)(const char *gfa_fn, const char *side, const AnyOpt *o);
	void (*write)(pg_graph_t *g, const char *side, const AnyOpt *o);
};
template <class O, void (*Init)(O *), int (*File)(const char *, const O *), void (*Write)(pg_graph_t *, const O *)>
static constexpr Calls calls()
{
	return { [](AnyOpt *o) { Init((O *)o); }, [](const char *fn, const char *, const AnyOpt *o) { return File(fn, (const O *)o); },
	         [](pg_graph_t *g, const char *, const AnyOpt *o) { Write(g, (const O *)o); } };
}
template <class O, void (*Init)(O *), int (*File)(const char *, const char *, const O *), void (*Write)(pg_graph_t *, const char *, const O *)>
static constexpr Calls calls_side()
{
	return { [](AnyOpt *o) { Init((O *)o); }, [](const char *fn, const char *side, const AnyOpt *o) { return File(fn, side, (const O *)o); },
	         [](pg_graph_t *g, const char *side, const AnyOpt *o) { Write(g, side, (const O *)o); } };
}

enum { MAX_ROWS = 11 };
enum HeadValue { HEAD_FILE, HEAD_ROW0 }; // the value of --NAME=X: the side file, or what the first row reads
struct Analysis {
	const char *name;      // the subcommand, and --NAME
	const char *head_form; // --NAME as the messages write it
	bool head_required;    // --NAME=X (and the subcommand cannot do without X either), not --NAME[=X]
	HeadValue head_value;
	const char *bare;      // what a --NAME without a value stands for, read by row 0 (nullptr: it leaves the value as it is)
	char file_letter;      // the side file of the subcommand (0: none)
	bool refusal_is_1;     // the library's "bad argument" (-3) on the PAF route ends with status 1, not 2
	Calls calls;
	void (*usage)(const AnyOpt &o); // of the subcommand, the defaults as pg_NAME_opt_init set them
	Row rows[MAX_ROWS];
};

// In the order in which --X refuses the ones before it (after --matrix and --call).  Oddities that are behaviour, kept as data:
// only the rows marked `extra` are refused without their --NAME (--curves-seed, --dist-metric, --assoc-*, --trait-perm, --trait-seed and
// --tree-* pass); a --NAME without a value after --NAME=X resets X for curves, dist and tree only (`bare`); the seeds and the counts of curves, assoc, trait and qtrait are read laxly; permanova's items are -T, gainloss
// resolves ties with -r and coevo with -e, phylosig has no tie rule; a row without a suffix exists for the subcommand only.
static const Analysis kAnalyses[] = {
	{ "curves", "--curves", false, HEAD_ROW0, "10", 0, false, calls<pg_curves_opt_t, pg_curves_opt_init, pg_curves_file, pg_write_curves>(),
	  [](const AnyOpt &o) {
		std::printf("Usage: pangene curves [options] <in.gfa>\nOptions:\n  -n INT   orders of the assemblies, the input order first [%d]\n"
		            "  -s INT   seed of the random orders [%u]\n", o.curves.n_perm, o.curves.seed); },
	  { late_count('n', offsetof(pg_curves_opt_t, n_perm), 1, M_MIN1, "needs at least one order"),
	    seed('s', offsetof(pg_curves_opt_t, seed)) } },
	{ "dist", "--dist", false, HEAD_ROW0, "gene", 0, false, calls<pg_dist_opt_t, pg_dist_opt_init, pg_dist_file, pg_write_dist>(),
	  [](const AnyOpt &) {
		std::printf("Usage: pangene dist [options] <in.gfa>\nOptions:\n  -t STR   items: gene (gene content) or adj (gene adjacencies of the walks) [gene]\n"
		            "  -m STR   metric: jaccard, shared or diff [jaccard]\n  -p       relaxed PHYLIP output\n"); },
	  { word('t', nullptr, offsetof(pg_dist_opt_t, type), W_TYPE, M_TYPE),
	    word('m', "metric", offsetof(pg_dist_opt_t, metric), W_DIST_METRIC, "must be jaccard, shared or diff"),
	    plain('p', nullptr, rd_flag, offsetof(pg_dist_opt_t, phylip), "") } },
	{ "assoc", "--assoc", false, HEAD_ROW0, nullptr, 0, false, calls<pg_assoc_opt_t, pg_assoc_opt_init, pg_assoc_file, pg_write_assoc>(),
	  [](const AnyOpt &o) {
		std::printf("Usage: pangene assoc [options] <in.gfa>\nOptions:\n  -r FLOAT  smallest |phi| of a reported pair, in [0, 1], read as per-mille [%g]\n"
		            "  -c INT    a gene takes part when it is present in >=INT and absent from >=INT assemblies [%d]\n"
		            "  -s STR    keep pos (co-occurring), neg (avoiding) or both [both]\n"
		            "  -x INT    give up when more than INT pairs pass [%lld]\n", o.assoc.min_phi, o.assoc.min_count, (long long)o.assoc.max_pair); },
	  { plain('r', nullptr, rd_unit, offsetof(pg_assoc_opt_t, min_phi), M_UNIT),
	    plain('c', "min-count", rd_atoi, offsetof(pg_assoc_opt_t, min_count), M_MIN1, false, 1),
	    word('s', "sign", offsetof(pg_assoc_opt_t, sign), W_SIGN, M_SIGN),
	    plain('x', nullptr, rd_atoll, offsetof(pg_assoc_opt_t, max_pair), M_NONNEG) } },
	{ "trait", "--trait=FILE", true, HEAD_FILE, nullptr, 't', false, calls_side<pg_trait_opt_t, pg_trait_opt_init, pg_trait_file, pg_write_trait>(),
	  [](const AnyOpt &o) {
		std::printf("Usage: pangene trait -t FILE [options] <in.gfa>\nOptions:\n  -t FILE   traits: a header line (any first field, one name per trait), then per line an assembly and 1, 0 or NA per trait\n"
		            "  -n INT    label permutations per trait; 0: none [%d]\n  -s INT    seed of the permutations [%u]\n"
		            "  -c INT    a gene is tested when it is present in >=INT and absent from >=INT assemblies [%d]\n"
		            "  -p FLOAT  print the genes with p_fisher <= FLOAT [%g]\n"
		            "  -L STR    lineage-aware test: the pairwise comparisons on the nj or upgma tree of all assemblies (gene content, jaccard);\n"
		            "            adds the columns pairs, supp, opp, p_pair_best and p_pair_worst [none]\n", o.trait.n_perm, o.trait.seed, o.trait.min_count, o.trait.max_p); },
	  { i32('n', "perm", offsetof(pg_trait_opt_t, n_perm), 0, INT31 - 1, M_PERM),
	    seed('s', offsetof(pg_trait_opt_t, seed)),
	    word('L', "lineage", offsetof(pg_trait_opt_t, lineage), W_LINEAGE, "must be nj or upgma", true),
	    plain('c', nullptr, rd_atoi, offsetof(pg_trait_opt_t, min_count), M_MIN1, false, 1),
	    plain('p', nullptr, rd_nonneg, offsetof(pg_trait_opt_t, max_p), "must be a number >= 0") } },
	{ "tree", "--tree", false, HEAD_ROW0, "gene", 0, false, calls<pg_tree_opt_t, pg_tree_opt_init, pg_tree_file, pg_write_tree>(),
	  [](const AnyOpt &) {
		std::printf("Usage: pangene tree [options] <in.gfa>\nOptions:\n  -t STR   items: gene (gene content) or adj (gene adjacencies of the walks) [gene]\n"
		            "  -m STR   distance: jaccard or diff [jaccard]\n"
		            "  -a STR   nj (neighbour-joining: unrooted, negative branch lengths are printed as they come) or upgma [nj]\n"
		            "  -b INT   bootstrap replicates over the items: inner nodes are labelled with their support in per cent [0]\n"
		            "  -s INT   seed of the bootstrap draws [0]\n"); },
	  { word('t', nullptr, offsetof(pg_tree_opt_t, type), W_TYPE, M_TYPE),
	    word('m', "metric", offsetof(pg_tree_opt_t, metric), W_METRIC, M_METRIC),
	    word('a', "method", offsetof(pg_tree_opt_t, method), W_METHOD, "must be nj or upgma"),
	    i32('b', "boot", offsetof(pg_tree_opt_t, n_boot), 0, INT31, M_INT31),
	    plain('s', "seed", rd_u32, offsetof(pg_tree_opt_t, seed), "must be in [0, 4294967295]") } },
	{ "qtrait", "--qtrait=FILE", true, HEAD_FILE, nullptr, 't', false, calls_side<pg_qtrait_opt_t, pg_qtrait_opt_init, pg_qtrait_file, pg_write_qtrait>(),
	  [](const AnyOpt &o) {
		std::printf("Usage: pangene qtrait -t FILE [options] <in.gfa>\nOptions:\n  -t FILE   traits: a header line (any first field, one name per trait), then per line an assembly and a number or NA per trait\n"
		            "  -n INT    permutations of the values per trait; 0: none [%d]\n  -s INT    seed of the permutations [%u]\n"
		            "  -c INT    a gene is tested when it is present in >=INT and absent from >=INT assemblies [%d]\n"
		            "  -p FLOAT  print the genes with p_wilcox <= FLOAT [%g]\n", o.qtrait.n_perm, o.qtrait.seed, o.qtrait.min_count, o.qtrait.max_p); },
	  { i32('n', "perm", offsetof(pg_qtrait_opt_t, n_perm), 0, INT31 - 1, M_PERM, true),
	    seed('s', offsetof(pg_qtrait_opt_t, seed), true),
	    plain('c', nullptr, rd_atoi, offsetof(pg_qtrait_opt_t, min_count), M_MIN1, false, 1),
	    plain('p', nullptr, rd_nonneg, offsetof(pg_qtrait_opt_t, max_p), "must be a number >= 0") } },
	{ "cluster", "--cluster=INT[-INT]", true, HEAD_ROW0, nullptr, 0, true, calls<pg_cluster_opt_t, pg_cluster_opt_init, pg_cluster_file, pg_write_cluster>(),
	  [](const AnyOpt &) {
		std::printf("Usage: pangene cluster -k INT[-INT] [options] <in.gfa>\nOptions:\n  -k INT[-INT]  clusters: one k, or a range whose k with the largest mean silhouette is printed in full\n"
		            "  -t STR   items: gene (gene content) or adj (gene adjacencies of the walks) [gene]\n"
		            "  -m STR   distance: jaccard or diff [jaccard]\n"
		            "  -i INT   swap iterations per k at the most [1000]\n"); },
	  { plain('k', nullptr, rd_cluster_range, offsetof(pg_cluster_opt_t, k_lo), "must be INT or INT-INT with 2 <= INT"),
	    word('t', "type", offsetof(pg_cluster_opt_t, type), W_TYPE, M_TYPE, true),
	    word('m', "metric", offsetof(pg_cluster_opt_t, metric), W_METRIC, M_METRIC, true),
	    i32('i', "iter", offsetof(pg_cluster_opt_t, max_iter), 0, INT31, M_INT31, true) } },
	{ "permanova", "--permanova=FILE", true, HEAD_FILE, nullptr, 't', false, calls_side<pg_permanova_opt_t, pg_permanova_opt_init, pg_permanova_file, pg_write_permanova>(),
	  [](const AnyOpt &o) {
		std::printf("Usage: pangene permanova -t FILE [options] <in.gfa>\nOptions:\n  -t FILE   traits: a header line (any first field, one name per trait), then per line an assembly and 1, 0 or NA per trait\n"
		            "  -T STR    items: gene (gene content) or adj (gene adjacencies of the walks) [gene]\n"
		            "  -m STR    distance: jaccard or diff [jaccard]\n"
		            "  -n INT    label permutations per trait; 0: none [%d]\n  -s INT    seed of the permutations [%u]\n", o.permanova.n_perm, o.permanova.seed); },
	  { word('T', "type", offsetof(pg_permanova_opt_t, type), W_TYPE, M_TYPE, true),
	    word('m', "metric", offsetof(pg_permanova_opt_t, metric), W_METRIC, M_METRIC, true),
	    i32('n', "perm", offsetof(pg_permanova_opt_t, n_perm), 0, INT31 - 1, M_PERM, true),
	    seed('s', offsetof(pg_permanova_opt_t, seed), true) } },
	{ "mantel", "--mantel", false, HEAD_FILE, nullptr, 'f', false, calls_side<pg_mantel_opt_t, pg_mantel_opt_init, pg_mantel_file, pg_write_mantel>(),
	  [](const AnyOpt &o) {
		std::printf("Usage: pangene mantel [options] <in.gfa>\nOptions:\n  -x SPEC   the first matrix: gene (gene content) or adj (gene adjacencies of the walks), ':', jaccard or diff [gene:jaccard]\n"
		            "  -y SPEC   the second matrix [adj:jaccard]\n"
		            "  -f FILE   the second matrix from FILE instead: the table or the PHYLIP form `pangene dist` prints\n"
		            "  -n INT    permutations of the assemblies; 0: none [%d]\n  -s INT    seed of the permutations [%u]\n", o.mantel.n_perm, o.mantel.seed); },
	  { spec('x', "x", offsetof(pg_mantel_opt_t, x_type), false),
	    spec('y', "y", offsetof(pg_mantel_opt_t, y_type), true), // (-y and the file both name the second matrix)
	    i32('n', "perm", offsetof(pg_mantel_opt_t, n_perm), 0, INT31 - 1, M_PERM, true),
	    seed('s', offsetof(pg_mantel_opt_t, seed), true) } },
	{ "gainloss", "--gainloss", false, HEAD_ROW0, nullptr, 0, false, calls<pg_gainloss_opt_t, pg_gainloss_opt_init, pg_gainloss_file, pg_write_gainloss>(),
	  [](const AnyOpt &o) {
		std::printf("Usage: pangene gainloss [options] <in.gfa>\nOptions:\n  -t STR   items: gene (gene content) or adj (gene adjacencies of the walks) [gene]\n"
		            "  -m STR   distance of the tree: jaccard or diff [jaccard]\n"
		            "  -a STR   tree: upgma, or nj rooted at its closing join, read as ((x, y), z): gains and losses depend on that reading [upgma]\n"
		            "  -g INT   cost of a gain, 1 to 255 [%d]\n  -l INT   cost of a loss, 1 to 255 [%d]\n"
		            "  -r STR   on a tie a change sits towards the tips (late) or towards the root (early) [late]\n"
		            "  -o STR   table: gene (per item: Present Cost Changes Gains Losses Root) or node (per branch: Leaves Present Gains Losses) [gene]\n"
		            "  -c INT   -o gene: print the items with at least INT changes [%d]\n", o.gainloss.gain, o.gainloss.loss, o.gainloss.min_changes); },
	  { word('o', nullptr, offsetof(pg_gainloss_opt_t, out), W_OUT, "must be gene or node"),
	    word('t', "type", offsetof(pg_gainloss_opt_t, type), W_TYPE, M_TYPE, true),
	    word('m', "metric", offsetof(pg_gainloss_opt_t, metric), W_METRIC, M_METRIC, true),
	    word('a', "method", offsetof(pg_gainloss_opt_t, method), W_METHOD, "must be upgma or nj", true),
	    i32('g', "gain", offsetof(pg_gainloss_opt_t, gain), 1, 255, M_COST, true),
	    i32('l', "loss", offsetof(pg_gainloss_opt_t, loss), 1, 255, M_COST, true),
	    word('r', "resolve", offsetof(pg_gainloss_opt_t, mode), W_MODE, M_MODE, true),
	    i32('c', "min", offsetof(pg_gainloss_opt_t, min_changes), 0, INT31, M_INT31, true) } },
	{ "coevo", "--coevo", false, HEAD_ROW0, nullptr, 0, false, calls<pg_coevo_opt_t, pg_coevo_opt_init, pg_coevo_file, pg_write_coevo>(),
	  [](const AnyOpt &o) {
		std::printf("Usage: pangene coevo [options] <in.gfa>\nOptions:\n  -t STR    items: gene (gene content) or adj (gene adjacencies of the walks) [gene]\n"
		            "  -m STR    distance of the tree: jaccard or diff [jaccard]\n"
		            "  -a STR    tree: upgma, or nj rooted at its closing join, read as ((x, y), z): the events depend on that reading [upgma]\n"
		            "  -g INT    cost of a gain, 1 to 255 [%d]\n  -l INT    cost of a loss, 1 to 255 [%d]\n"
		            "  -e STR    on a tie a change sits towards the tips (late) or towards the root (early) [late]\n"
		            "  -r FLOAT  smallest |r| of a reported pair, in [0, 1], read as per-mille [%g]\n"
		            "  -c INT    an item takes part with at least INT gains and losses; with 1 every pair of strain-specific genes of one assembly scores 1 [%d]\n"
		            "  -s STR    keep pos (same direction), neg (opposite direction) or both [both]\n"
		            "  -x INT    give up when more than INT pairs pass [%lld]\n", o.coevo.gain, o.coevo.loss, o.coevo.min_r, o.coevo.min_events, (long long)o.coevo.max_pair); },
	  { plain('r', nullptr, rd_unit, offsetof(pg_coevo_opt_t, min_r), M_UNIT),
	    word('t', "type", offsetof(pg_coevo_opt_t, type), W_TYPE, M_TYPE, true),
	    word('m', "metric", offsetof(pg_coevo_opt_t, metric), W_METRIC, M_METRIC, true),
	    word('a', "method", offsetof(pg_coevo_opt_t, method), W_METHOD, "must be upgma or nj", true),
	    i32('g', "gain", offsetof(pg_coevo_opt_t, gain), 1, 255, M_COST, true),
	    i32('l', "loss", offsetof(pg_coevo_opt_t, loss), 1, 255, M_COST, true),
	    word('e', "resolve", offsetof(pg_coevo_opt_t, mode), W_MODE, M_MODE, true),
	    i32('c', "min", offsetof(pg_coevo_opt_t, min_events), 1, INT31, M_MIN1, true),
	    word('s', "sign", offsetof(pg_coevo_opt_t, sign), W_SIGN, M_SIGN, true),
	    i64('x', "max", offsetof(pg_coevo_opt_t, max_pair), 0, LLONG_MAX, M_NONNEG, true) } },
	// (its lines in usage() wait for the next recording of the command-line transcript, which pins that text: the subcommand's own usage names both spellings)
	{ "phylosig", "--phylosig", false, HEAD_ROW0, nullptr, 0, false, calls<pg_phylosig_opt_t, pg_phylosig_opt_init, pg_phylosig_file, pg_write_phylosig>(),
	  [](const AnyOpt &o) {
		std::printf("Usage: pangene phylosig [options] <in.gfa>\n       pangene --phylosig[=INT] [--phylosig-NAME=VALUE ...] <in.paf> [...]   (INT: -n; NAME in parentheses below)\nOptions:\n"
		            "  -t STR    (type) items: gene (gene content) or adj (gene adjacencies of the walks) [gene]\n"
		            "  -m STR    (metric) distance of the tree: jaccard or diff [jaccard]\n"
		            "  -a STR    (method) tree: upgma, or nj rooted at its closing join, read as ((x, y), z): the costs depend on that reading unless -g and -l are equal [upgma]\n"
		            "  -g INT    (gain) cost of a gain, 1 to 255 [%d]\n  -l INT    (loss) cost of a loss, 1 to 255 [%d]\n"
		            "  -n INT    (--phylosig=INT) permutations of the tips: per item the random tip sets of its size on the same tree; 0: none [%d]\n"
		            "  -s INT    (seed) seed of the permutations [%u]\n"
		            "  -c INT    (min) an item is tested when it is present in >=INT and absent from >=INT assemblies [%d]\n"
		            "  -p FLOAT  (max-p) print the items with min(p_signal, p_scatter) <= FLOAT [%g]\n"
		            "Columns: p_signal is small when the item changes less often on the tree than chance (inherited down the lineages),\n"
		            "         p_scatter when more often (scattered over the tree); RI is the retention index\n",
		            o.phylosig.gain, o.phylosig.loss, o.phylosig.n_perm, o.phylosig.seed, o.phylosig.min_count, o.phylosig.max_p); },
	  { i32('n', nullptr, offsetof(pg_phylosig_opt_t, n_perm), 0, INT31 - 1, M_PERM),
	    word('t', "type", offsetof(pg_phylosig_opt_t, type), W_TYPE, M_TYPE, true),
	    word('m', "metric", offsetof(pg_phylosig_opt_t, metric), W_METRIC, M_METRIC, true),
	    word('a', "method", offsetof(pg_phylosig_opt_t, method), W_METHOD, "must be upgma or nj", true),
	    i32('g', "gain", offsetof(pg_phylosig_opt_t, gain), 1, 255, M_COST, true),
	    i32('l', "loss", offsetof(pg_phylosig_opt_t, loss), 1, 255, M_COST, true),
	    plain('s', "seed", rd_u32, offsetof(pg_phylosig_opt_t, seed), "must be in [0, 4294967295]", true),
	    i32('c', "min", offsetof(pg_phylosig_opt_t, min_count), 1, INT31, M_MIN1, true),
	    plain('p', "max-p", rd_nonneg, offsetof(pg_phylosig_opt_t, max_p), "must be a number >= 0", true) } },
	// (like phylosig: not in usage() until the transcript is recorded again)
	{ "pcoa", "--pcoa", false, HEAD_ROW0, nullptr, 0, false, calls<pg_pcoa_opt_t, pg_pcoa_opt_init, pg_pcoa_file, pg_write_pcoa>(),
	  [](const AnyOpt &o) {
		std::printf("Usage: pangene pcoa [options] <in.gfa>\n       pangene --pcoa[=INT] [--pcoa-NAME=VALUE ...] <in.paf> [...]   (INT: -k; NAME in parentheses below)\nOptions:\n"
		            "  -t STR   (type) items: gene (gene content) or adj (gene adjacencies of the walks) [gene]\n"
		            "  -m STR   (metric) distance: jaccard or diff [jaccard]\n"
		            "  -k INT   (--pcoa=INT) axes, 1 to 16; an axis is printed when its eigenvalue is above 1e-9 of the first [%d]\n"
		            "  -s INT   (seed) seed of the start vectors of the iteration [%u]\n"
		            "Principal coordinates (classical scaling) of the assemblies: EV lines, one per axis, then PC lines, one per assembly.\n"
		            "Explained = eigenvalue / trace, and the trace sums all eigenvalues, the negative ones included: for a distance that is\n"
		            "not Euclidean (diff, plain jaccard) it can overstate an axis' share.\n", o.pcoa.n_axis, o.pcoa.seed); },
	  { i32('k', nullptr, offsetof(pg_pcoa_opt_t, n_axis), 1, 16, "must be in [1, 16]"),
	    word('t', "type", offsetof(pg_pcoa_opt_t, type), W_TYPE, M_TYPE, true),
	    word('m', "metric", offsetof(pg_pcoa_opt_t, metric), W_METRIC, M_METRIC, true),
	    plain('s', "seed", rd_u32, offsetof(pg_pcoa_opt_t, seed), "must be in [0, 4294967295]", true) } },
	// (like phylosig and pcoa: not in usage() until the transcript is recorded again)
	{ "glm", "--glm=FILE", true, HEAD_FILE, nullptr, 't', false, calls_side<pg_glm_opt_t, pg_glm_opt_init, pg_glm_file, pg_write_glm>(),
	  [](const AnyOpt &o) {
		std::printf("Usage: pangene glm -t FILE [options] <in.gfa>\n       pangene --glm=FILE [--glm-NAME=VALUE ...] <in.paf> [...]   (NAME in parentheses below)\nOptions:\n"
		            "  -t FILE   traits: a header line (any first field, one name per trait), then per line an assembly and a value or NA per trait\n"
		            "  -y STR    (family) binary (values 1 and 0, logistic null model) or quant (numbers, least squares) [binary]\n"
		            "  -k INT    (axes) principal coordinates used as covariates, 0 to 13; 0: intercept only [%d]\n"
		            "  -T STR    (type) items of the distance: gene or adj [gene]; the items tested are the genes\n"
		            "  -m STR    (metric) distance: jaccard or diff [jaccard]\n"
		            "  -s INT    (seed) seed of the start vectors of the axes [%u]\n"
		            "  -c INT    (min) test genes with at least INT assemblies on either side [%d]\n"
		            "  -p FLOAT  (max-p) print genes with p <= FLOAT [%g]\n"
		            "Score test of every gene against each trait, adjusted for the axes of pangene pcoa: T lines, one per trait (Lambda is the\n"
		            "genomic inflation), then G lines.  A screening test: Beta is the one-step estimate for binary traits, and the axes adjust\n"
		            "for the structure the distance shows and for no other.\n", o.glm.n_axis, o.glm.seed, o.glm.min_count, o.glm.max_p); },
	  { word('y', "family", offsetof(pg_glm_opt_t, family), W_FAMILY, "must be binary or quant", true),
	    i32('k', "axes", offsetof(pg_glm_opt_t, n_axis), 0, 13, "must be in [0, 13]", true),
	    word('T', "type", offsetof(pg_glm_opt_t, type), W_TYPE, M_TYPE, true),
	    word('m', "metric", offsetof(pg_glm_opt_t, metric), W_METRIC, M_METRIC, true),
	    plain('s', "seed", rd_u32, offsetof(pg_glm_opt_t, seed), "must be in [0, 4294967295]", true),
	    i32('c', "min", offsetof(pg_glm_opt_t, min_count), 1, INT31, M_MIN1, true),
	    plain('p', "max-p", rd_nonneg, offsetof(pg_glm_opt_t, max_p), "must be a number >= 0", true) } },
	// (like phylosig, pcoa and glm: not in usage() until the transcript is recorded again)
	{ "rates", "--rates", false, HEAD_ROW0, nullptr, 0, true, calls<pg_rates_opt_t, pg_rates_opt_init, pg_rates_file, pg_write_rates>(),
	  [](const AnyOpt &) {
		std::printf("Usage: pangene rates [options] <in.gfa>\n       pangene --rates[=gene|node] [--rates-NAME=VALUE ...] <in.paf> [...]   (gene|node: -o; NAME in parentheses below)\nOptions:\n"
		            "  -t STR    (type) items: gene (gene content) or adj (gene adjacencies of the walks) [gene]\n"
		            "  -m STR    (metric) distance of the tree: jaccard or diff [jaccard]\n"
		            "  -a STR    (method) tree: upgma, or nj rooted in the middle of the third branch of its closing join ((x, y), z) [upgma]\n"
		            "  -g FLOAT  (gain) gain rate per item over the whole tree, in [1e-9, 1e9]; with -l: nothing is fitted [fitted]\n"
		            "  -l FLOAT  (loss) loss rate, as -g; one needs the other [fitted]\n"
		            "  -o STR    (--rates=STR) table: gene (per item: Present lnL Gains Losses Changes Root Rate LRT p_rate) or\n"
		            "            node (per branch: Leaves Length Present Gains Losses) [gene]\n"
		            "  -c FLOAT  (min) -o gene: print the items with Changes >= FLOAT [0]\n"
		            "Maximum-likelihood gain and loss rates of a two-state Markov model on the tree of the assemblies with its branch lengths,\n"
		            "corrected for the items nobody can observe.  The line after the header starts with # and holds the fit.  Gains and Losses are\n"
		            "the expected numbers of branches absent at the top and present at the bottom, and the reverse -- not the expected numbers of\n"
		            "events along the branches, which are larger.  Rate is the best of nine multipliers 2^-4 .. 2^4 of both rates, LRT and p_rate\n"
		            "compare it with 1: a screening value, not a maximum-likelihood rate per item.\n"); },
	  { word('o', nullptr, offsetof(pg_rates_opt_t, out), W_OUT, "must be gene or node"),
	    word('t', "type", offsetof(pg_rates_opt_t, type), W_TYPE, M_TYPE, true),
	    word('m', "metric", offsetof(pg_rates_opt_t, metric), W_METRIC, M_METRIC, true),
	    word('a', "method", offsetof(pg_rates_opt_t, method), W_METHOD, "must be upgma or nj", true),
	    plain('g', "gain", rd_rate, offsetof(pg_rates_opt_t, gain), "must be a number in [1e-9, 1e9]", true),
	    plain('l', "loss", rd_rate, offsetof(pg_rates_opt_t, loss), "must be a number in [1e-9, 1e9]", true),
	    plain('c', "min", rd_nonneg, offsetof(pg_rates_opt_t, min_changes), "must be a number >= 0", true) } },
};
enum { N_ANALYSES = sizeof(kAnalyses) / sizeof(kAnalyses[0]) };

static void *field_of(AnyOpt &o, const Row &r) { return (char *)&o + r.field; }

// `pangene NAME [options] <in.gfa>`
static int main_analysis(const Analysis &a, int argc, char *argv[])
{
	AnyOpt o;
	a.calls.init(&o);
	char letters[2 * MAX_ROWS + 3], *p = letters;
	if (a.file_letter) *p++ = a.file_letter, *p++ = ':';
	for (const Row *r = a.rows; r->read; ++r) if (r->letter) { *p++ = r->letter; if (r->read != rd_flag) *p++ = ':'; }
	*p = 0;
	const char *side = nullptr;
	const Row *no_file = nullptr;
	bool have_row0 = false;
	int c;
	while ((c = getopt(argc, argv, letters)) >= 0) {
		if (c == a.file_letter) { side = optarg; continue; }
		const Row *r = a.rows;
		while (r->read && r->letter != c) ++r;
		if (r->read == nullptr) return 1; // (getopt has said what is wrong)
		if (r->no_file) no_file = r;
		const bool ok = r->read(optarg, field_of(o, *r), *r);
		if (!ok && !r->late) { std::fprintf(stderr, "ERROR: -%c %s\n", c, r->msg); return 1; }
		if (r == a.rows) have_row0 = ok;
	}
	for (const Row *r = a.rows; r->read; ++r)
		if (r->late && *(const int32_t *)field_of(o, *r) < r->lo) { std::fprintf(stderr, "ERROR: -%c %s\n", r->letter, r->msg); return 1; }
	if (argc - optind < 1) { a.usage(o); return 0; }
	if (a.head_required && !(a.head_value == HEAD_FILE ? side != nullptr : have_row0)) {
		std::fprintf(stderr, "ERROR: pangene %s needs -%c %s\n", a.name, a.head_value == HEAD_FILE ? a.file_letter : a.rows[0].letter, std::strchr(a.head_form, '=') + 1);
		return 1;
	}
	if (no_file && side) { std::fprintf(stderr, "ERROR: -%c cannot be combined with -%c\n", no_file->letter, a.file_letter); return 1; }
	return a.calls.file(argv[optind], side, &o) == 0 ? 0 : 1;
}

// `pangene --NAME[=X] --NAME-suffix=X ...`: what the options of one analysis have said so far.  Every analysis keeps its own, as a
// --NAME-suffix may come before its --NAME or, for the rows that are not `extra`, without it.
struct Parsed { AnyOpt opt; const char *side = nullptr; bool asked = false, extra = false; const Row *no_file = nullptr; };

// the codes getopt_long returns for them: LONG_BASE + analysis * LONG_STRIDE for --NAME, + 1 + row for --NAME-suffix
enum { LONG_BASE = 1000, LONG_STRIDE = MAX_ROWS + 1, N_FIXED_LONG = 8 };
static struct option g_long[N_FIXED_LONG + N_ANALYSES * LONG_STRIDE + 1];
static char g_long_name[N_ANALYSES * MAX_ROWS][32];

static void long_options_init() // the reference's own options around the table's, in the order of the usage text
{
	static const struct option first[] = { { "bed", optional_argument, nullptr, 301 }, { "ori-sc", no_argument, nullptr, 302 }, { "matrix", optional_argument, nullptr, 303 },
		{ "call", no_argument, nullptr, 305 } };
	static const struct option last[] = { { "gpus", required_argument, nullptr, 304 }, { "procs", required_argument, nullptr, 304 }, { "version", no_argument, nullptr, 401 },
		{ nullptr, 0, nullptr, 0 } };
	struct option *lo = g_long;
	int n_name = 0;
	for (const struct option &f : first) *lo++ = f;
	for (int i = 0; i < N_ANALYSES; ++i) {
		const Analysis &a = kAnalyses[i];
		*lo++ = { a.name, a.head_required ? required_argument : optional_argument, nullptr, LONG_BASE + i * LONG_STRIDE };
		for (int k = 0; a.rows[k].read; ++k) {
			if (a.rows[k].suffix == nullptr) continue;
			std::snprintf(g_long_name[n_name], sizeof(g_long_name[0]), "%s-%s", a.name, a.rows[k].suffix);
			*lo++ = { g_long_name[n_name++], required_argument, nullptr, LONG_BASE + i * LONG_STRIDE + 1 + k };
		}
	}
	for (const struct option &l : last) *lo++ = l;
}

static bool long_option(int code, const char *arg, Parsed *parsed) // false: refused, and said why
{
	const int i = (code - LONG_BASE) / LONG_STRIDE, k = (code - LONG_BASE) % LONG_STRIDE - 1;
	const Analysis &a = kAnalyses[i];
	Parsed &p = parsed[i];
	const Row *r = k < 0 ? a.rows : &a.rows[k];
	if (k < 0) { // --NAME[=X]
		p.asked = true;
		if (a.head_value == HEAD_FILE) p.side = arg;
		if (a.head_value == HEAD_FILE) return true;
		if (arg == nullptr && (arg = a.bare) == nullptr) return true; // (a later --curves, --dist or --tree without a value is the default again; --assoc, --gainloss, --coevo, --phylosig and --pcoa keep what an earlier one said)
	} else {
		if (r->extra) p.extra = true;
		if (r->no_file) p.no_file = r;
	}
	if (r->read(arg, field_of(p.opt, *r), *r)) return true;
	std::fprintf(stderr, "ERROR: --%s%s%s %s\n", a.name, k < 0 ? "" : "-", k < 0 ? "" : r->suffix, r->long_msg ? r->long_msg : r->msg);
	return false;
}

// After parsing: --X cannot be combined with anything before it in the table (--matrix and --call come first), and the `extra` rows need
// their --X.  One analysis after the other, so that of two mistakes the one reported is the one that always was.
static bool check_analyses(const Parsed *parsed, bool matrix, bool call, int &which) // false: refused, and said why; which: the one asked for, or -1
{
	const char *before[2 + N_ANALYSES] = { "matrix", "call" }; // (--matrix --call together pass, and the matrix is printed)
	int n_before = 2;
	bool any = matrix || call;
	which = -1;
	for (int i = 0; i < N_ANALYSES; ++i) {
		const Analysis &a = kAnalyses[i];
		const Parsed &p = parsed[i];
		if (p.asked && any) {
			std::fprintf(stderr, "ERROR: --%s cannot be combined with", a.name);
			for (int k = 0; k < n_before; ++k) std::fprintf(stderr, "%s--%s", k == 0 ? " " : k == n_before - 1 ? " or " : ", ", before[k]);
			std::fputc('\n', stderr);
			return false;
		}
		if (p.extra && !p.asked) {
			int n = 0, k = 0;
			for (const Row *r = a.rows; r->read; ++r) n += r->extra;
			std::fprintf(stderr, "ERROR:");
			for (const Row *r = a.rows; r->read; ++r) if (r->extra) { std::fprintf(stderr, "%s--%s-%s", k == 0 ? " " : k == n - 1 ? " and " : ", ", a.name, r->suffix); ++k; }
			std::fprintf(stderr, " %s %s\n", n == 1 ? "needs" : "need", a.head_form);
			return false;
		}
		if (p.no_file && p.side) { std::fprintf(stderr, "ERROR: --%s-%s cannot be combined with --%s=FILE\n", a.name, p.no_file->suffix, a.name); return false; }
		if (p.asked) which = i, any = true;
		before[n_before++] = a.name;
	}
	return true;
}

// ---------------------------------------------------------------------------------------------------------------
// `pangene --gpus N`: main.c:117-142 for N devices of one node.  The command forks N - 1 workers BEFORE anything touches the GPU;
// rank r takes device r and the r-th contiguous block of the PAF files (so that the ranks' W / BED lines, concatenated in rank
// order, are in command-line order) and registers the names of the other files (ids as in a sequential read).  The exchange is
// RCCL on the kernels' stream (the 128-byte id travels through a pipe); on a backend without a device (the oracle host of the
// tests) it is a shared-memory region mapped before the fork.  Rank 0 prints the graph; every rank writes the lines of its own
// genomes to a temporary file that rank 0 copies to stdout in rank order.
// ---------------------------------------------------------------------------------------------------------------
// what to print instead of the graph: the matrix, the bubbles, or one analysis with its options and its side file
struct Output { int matrix = 0; bool call = false; const Analysis *analysis = nullptr; AnyOpt opt; const char *side = nullptr; }; // matrix: 1 presence, 2 counts

static int run_path(pg_opt_t &opt, int n_files, char **files, const uint8_t *ids_only, const Output &o, bool graph_lines, bool own_lines, int device = -1)
{
	// PANGENE_TIMING=1: where the wall time of the command goes (stderr: the line bench.py's cli leg reads), beside the library's own lines
	const bool timing = std::getenv("PANGENE_TIMING") != nullptr;
	const double t0 = pg_realtime();
	// (Tried: HIP initialisation + code-object load on a helper thread while the files are parsed -- pg_device_warm().  The runtime's
	// start-up maps and registers memory for ~0.3 s and every one of those calls stalls the page faults of the parser threads of the
	// same address space: parsing 100 files took 0.30 s instead of 0.05 s and the command got slower, 0.55 s against 0.46 s.  So the
	// device comes up when pg_post_process first needs it; `device_warm_s` below is that start-up, measured on its own.)
	pg_data_t *d = pg_data_init();
	pg_read_paf_batch(&opt, d, n_files, files, ids_only, 0); // parallel parse, ids as in sequential pg_read_paf calls
	const double t1 = pg_realtime();
	if (device >= 0) pg_set_device(device);
	if (timing) pg_device_warm(); // (only to itemise it: pg_post_process would pay it otherwise)
	const double t2 = pg_realtime();
	const double t_warm = t2 - t1;
	pg_post_process(&opt, d);
	const double t3 = pg_realtime();
	double t4 = t3;
	int rc = 0;
	if (pg_last_error()) rc = 2;
	else if (opt.flag & PG_F_WRITE_BED_RAW) { if (own_lines) pg_write_bed(d, 0); }
	else {
		pg_graph_t *g = pg_graph_init(d);
		pg_graph_gen(&opt, g);
		t4 = pg_realtime();
		if (pg_last_error()) rc = 2;
		else if (o.matrix) pg_write_matrix(g, o.matrix == 2);
		else if (o.call) { pg_call_opt_t co; pg_call_opt_init(&co); pg_write_call(g, &co); if (pg_last_error()) rc = 2; }
		else if (o.analysis) {
			o.analysis->calls.write(g, o.side, &o.opt);
			if (pg_last_error()) rc = o.analysis->refusal_is_1 && pg_last_error() == -3 ? 1 : 2; // (cluster's -3, PGA_ERR_ARG: a k outside [2, assemblies - 1] or fewer than 3 assemblies; rates': one rate without the other -- a refusal, as on the subcommand)
		}
		else if (opt.flag & PG_F_WRITE_BED_WALK) { if (own_lines) pg_write_bed(d, 1); }
		else if (opt.flag & PG_F_WRITE_BED_FLAG) { if (own_lines) pg_write_bed(d, 0); }
		else {
			if (graph_lines) { pg_write_graph(g); std::fflush(stdout); }
			if (own_lines && !(opt.flag & PG_F_WRITE_NO_WALK)) pg_write_walk(g);
		}
		pg_graph_destroy(g);
	}
	std::fflush(stdout);
	const double t5 = pg_realtime();
	pg_data_destroy(d);
	if (timing) std::fprintf(stderr, "[cli_timing] {\"parse_s\": %.4f, \"device_warm_s\": %.4f, \"post_process_s\": %.4f, \"graph_gen_s\": %.4f, \"write_s\": %.4f, \"teardown_s\": %.4f}\n",
	                         t1 - t0, t_warm, t3 - t2, t4 - t3, t5 - t4, pg_realtime() - t5);
	return rc;
}

static bool read_all(int fd, void *buf, size_t n) { char *p = (char *)buf; while (n) { ssize_t k = read(fd, p, n); if (k <= 0) return false; p += k, n -= (size_t)k; } return true; }
static bool write_all(int fd, const void *buf, size_t n) { const char *p = (const char *)buf; while (n) { ssize_t k = write(fd, p, n); if (k <= 0) return false; p += k, n -= (size_t)k; } return true; }

// what a signal handler / the watchdog needs to take the whole command down: the workers' pids and the temporary files
static std::vector<pid_t> g_kids;
static std::vector<std::string> g_tmp;
static std::atomic<int> g_kid_failed{0}; // a worker ended with an error while rank 0 was still at work

static void take_down(bool unlink_tmp)
{
	for (pid_t p : g_kids) if (p > 0) kill(p, SIGKILL);
	if (unlink_tmp) for (const std::string &t : g_tmp) unlink(t.c_str());
}
static void on_signal(int sig) { take_down(true); _exit(128 + sig); }

// Files of rank r = a contiguous block of the command line (the ranks' W / BED lines, concatenated in rank order, are then in
// command-line order), cut so that the blocks carry about the same number of HITS.  The hits of a file are not
// known before it is parsed; its size is (one PAF line is one alignment; a .gz counts five times its size, as in the reader).
static std::vector<int> partition_files(int W, int n_files, char **files)
{
	std::vector<double> w((size_t)n_files, 1.0);
	double tot = 0;
	for (int i = 0; i < n_files; ++i) {
		struct stat sb;
		const size_t len = std::strlen(files[i]);
		if (stat(files[i], &sb) == 0 && sb.st_size > 0) w[(size_t)i] = (double)sb.st_size * (len > 3 && std::strcmp(files[i] + len - 3, ".gz") == 0 ? 5.0 : 1.0);
		tot += w[(size_t)i];
	}
	std::vector<int> cut((size_t)W + 1, n_files);
	cut[0] = 0;
	double acc = 0;
	int r = 1;
	for (int i = 0; i < n_files && r < W; ++i) { // rank r starts at the first file at which the weight before it reaches r / W of the total
		while (r < W && acc >= tot * r / W) cut[(size_t)r++] = i;
		acc += w[(size_t)i];
	}
	return cut;
}

static int run_sharded(pg_opt_t &opt, int W, int n_files, char **files, const Output &o)
{
	const char *whole = o.matrix ? "matrix" : o.call ? "call" : o.analysis ? o.analysis->name : nullptr;
	if (whole) { std::fprintf(stderr, "ERROR: --%s needs every genome in one process; run it without --gpus\n", whole); return 1; }
	const bool dev = pg_backend_is_device() != 0;
	typedef int (*uid_fn)(void *); typedef int (*init_fn)(int32_t, int32_t, const void *); typedef int (*fin_fn)(void);
	uid_fn rccl_uid = nullptr; init_fn rccl_init = nullptr; fin_fn rccl_fin = nullptr;
	void *region = nullptr;
	if (dev) { // bound at run time: only the HIP build of the library has them
		rccl_uid = (uid_fn)dlsym(RTLD_DEFAULT, "pg_rccl_unique_id"), rccl_init = (init_fn)dlsym(RTLD_DEFAULT, "pg_rccl_init"), rccl_fin = (fin_fn)dlsym(RTLD_DEFAULT, "pg_rccl_finalize");
		if (!rccl_uid || !rccl_init) { std::fprintf(stderr, "ERROR: this build of the library has no RCCL exchange\n"); return 1; }
	} else if ((region = pg_shm_create(W, (int64_t)16 << 20)) == nullptr) { std::fprintf(stderr, "ERROR: cannot map the exchange region\n"); return 1; }
	const std::vector<int> cut = partition_files(W, n_files, files);
	std::vector<std::string> &tmp = g_tmp;
	tmp.assign((size_t)W, std::string());
	std::vector<int> id_pipe((size_t)W * 2, -1), st_pipe((size_t)W * 2, -1);
	std::vector<pid_t> &kid = g_kids;
	kid.assign((size_t)W, 0);
	const char *td = std::getenv("TMPDIR");
	for (int r = 0; r < W; ++r) {
		std::string t = std::string(td && *td ? td : "/tmp") + "/pangene_rank" + std::to_string(r) + "_XXXXXX";
		const int fd = mkstemp(&t[0]);
		if (fd < 0) { std::fprintf(stderr, "ERROR: cannot create a temporary file for rank %d\n", r); take_down(true); return 1; }
		close(fd);
		tmp[(size_t)r] = t;
		if (r && (pipe(&id_pipe[(size_t)r * 2]) != 0 || pipe(&st_pipe[(size_t)r * 2]) != 0)) { std::fprintf(stderr, "ERROR: pipe()\n"); take_down(true); return 1; }
	}
	std::fflush(stdout); std::fflush(stderr);
	const pid_t parent = getpid();
	int rank = 0;
	for (int r = 1; r < W; ++r) {
		const pid_t p = fork();
		if (p < 0) { std::fprintf(stderr, "ERROR: fork()\n"); take_down(true); return 1; }
		if (p == 0) {
			rank = r;
			prctl(PR_SET_PDEATHSIG, SIGKILL); // a worker never outlives rank 0 (it would wait in a collective for ever)
			if (getppid() != parent) _exit(3);
			for (int k = 1; k < W; ++k) { // the other workers' pipes are none of this one's business (an inherited write end would keep a dead rank 0's pipe open)
				if (k == r) continue;
				for (int e = 0; e < 2; ++e) { if (id_pipe[(size_t)k * 2 + e] >= 0) close(id_pipe[(size_t)k * 2 + e]); if (st_pipe[(size_t)k * 2 + e] >= 0) close(st_pipe[(size_t)k * 2 + e]); }
			}
			std::fill(kid.begin(), kid.end(), 0);
			break;
		}
		kid[(size_t)r] = p;
	}
	if (rank == 0) { signal(SIGINT, on_signal); signal(SIGTERM, on_signal); signal(SIGHUP, on_signal); }
	std::vector<uint8_t> ids_only((size_t)n_files, 1);
	for (int i = cut[(size_t)rank]; i < cut[(size_t)rank + 1]; ++i) ids_only[(size_t)i] = 0;
	int rc = 0;
	if (dev && pg_set_device(rank) != 0) { std::fprintf(stderr, "[E::pangene] rank %d: no HIP device %d\n", rank, rank); rc = 3; }
	// bootstrap: rank 0 hands the id out and hears from every worker before anybody enters the communicator
	unsigned char id[128] = { 0 };
	if (rank == 0) {
		if (dev && rc == 0 && rccl_uid(id) != 0) rc = 3;
		unsigned char ok = rc == 0 ? 1 : 0;
		for (int r = 1; r < W; ++r) {
			close(id_pipe[(size_t)r * 2]), close(st_pipe[(size_t)r * 2 + 1]);
			if (!write_all(id_pipe[(size_t)r * 2 + 1], &ok, 1) || !write_all(id_pipe[(size_t)r * 2 + 1], id, sizeof(id))) ok = 0;
		}
		for (int r = 1; r < W; ++r) { unsigned char s = 0; if (!read_all(st_pipe[(size_t)r * 2], &s, 1) || !s) ok = 0; }
		for (int r = 1; r < W; ++r) write_all(id_pipe[(size_t)r * 2 + 1], &ok, 1); // go / no go
		if (!ok) { for (int r = 1; r < W; ++r) { int st; waitpid(kid[(size_t)r], &st, 0); kid[(size_t)r] = 0; } take_down(true); return 3; } // (reaped: take_down must not signal a pid the system may have given to somebody else)
	} else {
		close(id_pipe[(size_t)rank * 2 + 1]), close(st_pipe[(size_t)rank * 2]);
		unsigned char ok = 0, go = 0, mine = rc == 0 ? 1 : 0;
		if (!read_all(id_pipe[(size_t)rank * 2], &ok, 1) || !read_all(id_pipe[(size_t)rank * 2], id, sizeof(id))) ok = 0;
		if (!ok) mine = 0;
		write_all(st_pipe[(size_t)rank * 2 + 1], &mine, 1);
		if (!read_all(id_pipe[(size_t)rank * 2], &go, 1) || !go) _exit(3);
		opt.flag &= ~PG_F_WRITE_VTX_SEL; // (-G lines come from rank 0 only)
		if (pg_verbose > 1) pg_verbose = 1; // one log, rank 0's (the ROUTES of a sharded run follow a level all ranks agree on: graph_driver.cpp route_v)
	}
	// From here on a rank that fails alone would leave the others waiting in a collective for ever.  Rank 0 watches its workers: the
	// first one that ends with an error (or by a signal) takes the command down -- workers and temporary files -- with status 2.
	std::atomic<bool> watch_on{rank == 0};
	std::vector<int> kid_status((size_t)W, -1); // exit status of the workers the watchdog has reaped
	std::thread watchdog;
	if (rank == 0 && W > 1) watchdog = std::thread([&]() {
		int left = W - 1;
		while (watch_on.load() && left > 0) {
			bool any = false;
			for (int r = 1; r < W; ++r) {
				if (kid[(size_t)r] <= 0 || kid_status[(size_t)r] >= 0) continue;
				int st = 0;
				const pid_t p = waitpid(kid[(size_t)r], &st, WNOHANG);
				if (p != kid[(size_t)r]) continue;
				any = true, --left;
				kid_status[(size_t)r] = (WIFEXITED(st) && WEXITSTATUS(st) == 0) ? 0 : 1;
				if (kid_status[(size_t)r] == 0) kid[(size_t)r] = 0; // (reaped: the pid is nobody's any more)
				else {
					std::fprintf(stderr, "[E::pangene] rank %d failed; stopping the other ranks\n", r);
					g_kid_failed.store(1);
					kid[(size_t)r] = 0;
					take_down(true);
					_exit(2);
				}
			}
			if (!any) usleep(20000);
		}
	});
	if ((dev ? rccl_init(rank, W, id) : pg_shm_init(region, rank)) != 0) { std::fprintf(stderr, "[E::pangene] rank %d: cannot join the exchange\n", rank); rc = 3; }
	if (const char *fr = std::getenv("PANGENE_FAULT_RANK")) if (std::atoi(fr) == rank) { std::fprintf(stderr, "[E::pangene] rank %d: injected fault (PANGENE_FAULT_RANK)\n", rank); rc = 7; } // (tests: a rank that fails alone)
	if (rc == 0) {
		if (rank) { if (pg_set_output(tmp[(size_t)rank].c_str()) != 0) rc = 3; }
		if (rc == 0) rc = run_path(opt, n_files, files, ids_only.data(), o, rank == 0, true, dev ? rank : -1);
		if (rank) pg_set_output(nullptr);
	}
	if (rank) { // (no RCCL teardown on a failed rank: the others may be inside a collective -- rank 0's watchdog ends them)
		if (rc == 0 && dev && rccl_fin) rccl_fin();
		std::fflush(stderr);
		_exit(rc);
	}
	if (rc != 0) { // rank 0 failed: the workers may be waiting for it
		watch_on.store(false);
		if (watchdog.joinable()) watchdog.join();
		take_down(true);
		return rc;
	}
	if (dev && rccl_fin) rccl_fin();
	std::fflush(stdout);
	watch_on.store(false);
	if (watchdog.joinable()) watchdog.join();
	for (int r = 1; r < W; ++r) {
		if (kid_status[(size_t)r] == 0) continue; // (reaped by the watchdog, ended well)
		int st = 0;
		if (kid[(size_t)r] <= 0 || waitpid(kid[(size_t)r], &st, 0) < 0 || !WIFEXITED(st) || WEXITSTATUS(st) != 0) { std::fprintf(stderr, "[E::pangene] rank %d failed\n", r); rc = rc ? rc : 2; }
		kid[(size_t)r] = 0;
	}
	for (int r = 1; r < W && rc == 0; ++r) { // the other ranks' lines, in rank (= command-line) order
		FILE *fp = std::fopen(tmp[(size_t)r].c_str(), "rb");
		if (!fp) { rc = 2; break; }
		char buf[1 << 16];
		size_t k;
		while ((k = std::fread(buf, 1, sizeof(buf), fp)) > 0) std::fwrite(buf, 1, k, stdout);
		std::fclose(fp);
	}
	take_down(true);
	return rc;
}

int main(int argc, char *argv[])
{
	if (argc >= 2 && std::strcmp(argv[1], "gfa2matrix") == 0) return main_gfa2matrix(argc - 1, argv + 1);
	if (argc >= 2 && std::strcmp(argv[1], "call") == 0) return main_call(argc - 1, argv + 1);
	for (const Analysis &a : kAnalyses) if (argc >= 2 && std::strcmp(argv[1], a.name) == 0) return main_analysis(a, argc - 1, argv + 1);
	int n_gpus = 1;
	Output o;
	Parsed parsed[N_ANALYSES];
	for (int i = 0; i < N_ANALYSES; ++i) kAnalyses[i].calls.init(&parsed[i].opt);
	long_options_init();
	pg_opt_t opt;
	pg_opt_init(&opt);
	int c;
	while ((c = getopt_long(argc, argv, "d:e:l:f:g:p:b:B:y:Fr:c:a:wv:GD:C:T:X:I:P:m:JOSE", g_long, nullptr)) >= 0) {
		switch (c) {
		case 'd': opt.gene_delim = *optarg; break;
		case 'X': opt.excl = pg_read_list_dict(optarg); break;
		case 'I': opt.incl = pg_read_list_dict(optarg); break;
		case 'P': opt.preferred = pg_read_list_dict(optarg); break;
		case 'e': opt.min_prot_iden = std::atof(optarg); break;
		case 'l': opt.min_prot_ratio = std::atof(optarg); break;
		case 'm': opt.score_adj_coef = std::atof(optarg); break;
		case 'f': opt.min_ov_ratio = std::atof(optarg); break;
		case 'p': opt.min_vertex_ratio = std::atof(optarg); break;
		case 'c': opt.max_avg_occ = std::atoi(optarg); break;
		case 'g': opt.max_degree = std::atoi(optarg); break;
		case 'r': opt.max_dist_loci = std::atoi(optarg); break;
		case 'J': opt.flag |= PG_F_NO_JOINT_PSEUDO; break;
		case 'E': opt.flag |= PG_F_DROP_SGL_EXON; break;
		case 'b': opt.branch_diff = std::atof(optarg); break;
		case 'B': opt.branch_diff_cut = std::atof(optarg); break;
		case 'y': opt.branch_diff_dist = std::atof(optarg); break;
		case 'T': opt.n_branch_flt = (int32_t)std::atof(optarg); break;
		case 'a': opt.min_arc_cnt = std::atoi(optarg); break;
		case 'F': opt.flag |= PG_F_FRAG_MODE; break;
		case 'D': opt.local_dist = (int32_t)parse_num(optarg); break;
		case 'C': opt.local_count = std::atoi(optarg); break;
		case 'S': opt.flag |= PG_F_CHECK_STRAND; break;
		case 'w': opt.flag |= PG_F_WRITE_NO_WALK; break;
		case 'G': opt.flag |= PG_F_WRITE_VTX_SEL; break;
		case 'v': pg_verbose = std::atoi(optarg); break;
		case 'O': break; // accepted and ignored, as in the reference
		case 301:
			if (optarg == nullptr || std::strcmp(optarg, "walk") == 0) opt.flag |= PG_F_WRITE_BED_WALK;
			else if (std::strcmp(optarg, "raw") == 0) opt.flag |= PG_F_WRITE_BED_RAW;
			else if (std::strcmp(optarg, "flag") == 0) opt.flag |= PG_F_WRITE_BED_FLAG;
			else { std::fprintf(stderr, "ERROR: unrecognized --bed argument. Should be 'raw' or 'walk'.\n"); return 1; }
			break;
		case 302: opt.flag |= PG_F_ORI_FOR_BRANCH; break;
		case 303: o.matrix = (optarg && std::strcmp(optarg, "count") == 0) ? 2 : 1; break;
		case 304: n_gpus = std::atoi(optarg); break;
		case 305: o.call = true; break;
		case 401: std::puts(PG_VERSION); return 0;
		default:
			if (c >= LONG_BASE && !long_option(c, optarg, parsed)) return 1;
			break;
		}
	}
	if (argc - optind < 1) return usage(stderr, &opt);
	int which;
	if (!check_analyses(parsed, o.matrix != 0, o.call, which)) return 1;
	if (which >= 0) o.analysis = &kAnalyses[which], o.opt = parsed[which].opt, o.side = parsed[which].side;
	int rc;
	if (n_gpus > 1) {
		rc = run_sharded(opt, n_gpus, argc - optind, argv + optind, o);
	} else rc = run_path(opt, argc - optind, argv + optind, nullptr, o, true, true);
	if (opt.excl) pg_dict_destroy(opt.excl);
	if (opt.incl) pg_dict_destroy(opt.incl);
	if (opt.preferred) pg_dict_destroy(opt.preferred);
	if (pg_verbose >= 3) {
		struct rusage r;
		getrusage(RUSAGE_SELF, &r);
		std::fprintf(stderr, "[M::%s] Version: %s\n[M::%s] CMD:", __func__, PG_VERSION, __func__);
		for (int i = 0; i < argc; ++i) std::fprintf(stderr, " %s", argv[i]);
		std::fprintf(stderr, "\n[M::%s] stages A+B+C: %.3f sec for %ld hits; peak RSS: %.3f GB\n", __func__, pg_last_path_seconds(),
		             (long)pg_last_path_hits(), r.ru_maxrss / 1024.0 / 1024.0);
	}
	return rc;
}
