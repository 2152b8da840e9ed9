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

// `pangene curves`: pan / core / new / unique accumulation curves of the matrix `pangene gfa2matrix` prints for the same GFA
static int main_curves(int argc, char *argv[])
{
	pg_curves_opt_t o;
	pg_curves_opt_init(&o);
	int c;
	while ((c = getopt(argc, argv, "n:s:")) >= 0) {
		if (c == 'n') o.n_perm = std::atoi(optarg);
		else if (c == 's') o.seed = (uint32_t)std::strtoul(optarg, nullptr, 10);
		else return 1;
	}
	if (o.n_perm < 1) { std::fprintf(stderr, "ERROR: -n must be at least 1\n"); return 1; }
	if (argc - optind < 1) {
		std::printf("Usage: pangene curves [options] <in.gfa>\nOptions:\n  -n INT   orders of the assemblies, the input order first [%d]\n"
		            "  -s INT   seed of the random orders [%u]\n", o.n_perm, o.seed);
		return 0;
	}
	return pg_curves_file(argv[optind], &o) == 0 ? 0 : 1;
}

static int dist_type(const char *s) { return std::strcmp(s, "gene") == 0 ? PG_DIST_GENE : std::strcmp(s, "adj") == 0 ? PG_DIST_ADJ : -1; }
static int dist_metric(const char *s)
{
	return std::strcmp(s, "jaccard") == 0 ? PG_DIST_JACCARD : std::strcmp(s, "shared") == 0 ? PG_DIST_SHARED : std::strcmp(s, "diff") == 0 ? PG_DIST_DIFF : -1;
}

// `pangene dist`: pairwise distances of the assemblies of a GFA file over their genes or their gene adjacencies
static int main_dist(int argc, char *argv[])
{
	pg_dist_opt_t o;
	pg_dist_opt_init(&o);
	int c;
	while ((c = getopt(argc, argv, "t:m:p")) >= 0) {
		if (c == 't') { if ((o.type = dist_type(optarg)) < 0) { std::fprintf(stderr, "ERROR: -t must be gene or adj\n"); return 1; } }
		else if (c == 'm') { if ((o.metric = dist_metric(optarg)) < 0) { std::fprintf(stderr, "ERROR: -m must be jaccard, shared or diff\n"); return 1; } }
		else if (c == 'p') o.phylip = 1;
		else return 1;
	}
	if (argc - optind < 1) {
		std::printf("Usage: pangene dist [options] <in.gfa>\nOptions:\n  -t STR   items: gene (gene content) or adj (gene adjacencies of the walks) [gene]\n"
		            "  -m STR   metric: jaccard, shared or diff [jaccard]\n  -p       relaxed PHYLIP output\n");
		return 0;
	}
	return pg_dist_file(argv[optind], &o) == 0 ? 0 : 1;
}

static int tree_metric(const char *s) { return std::strcmp(s, "jaccard") == 0 ? PG_DIST_JACCARD : std::strcmp(s, "diff") == 0 ? PG_DIST_DIFF : -1; }
static int tree_method(const char *s) { return std::strcmp(s, "nj") == 0 ? PG_TREE_NJ : std::strcmp(s, "upgma") == 0 ? PG_TREE_UPGMA : -1; }
static bool tree_boot(const char *s, int32_t &v) // a whole number of replicates
{
	char *end = nullptr;
	const long long x = std::strtoll(s, &end, 10);
	if (end == s || *end != 0 || x < 0 || x > 2147483647ll) return false;
	v = (int32_t)x;
	return true;
}
static bool tree_seed_arg(const char *s, uint32_t &v) // a whole number that fits 32 bits; digits only (strtoull alone would take "-1" and " 7")
{
	char *end = nullptr;
	if (*s < '0' || *s > '9') return false;
	const unsigned long long x = std::strtoull(s, &end, 10);
	if (*end != 0 || end - s > 10 || x > 4294967295ull) return false;
	v = (uint32_t)x;
	return true;
}

// `pangene tree`: a neighbour-joining or UPGMA tree of the assemblies of a GFA file from the distances `pangene dist` prints
static int main_tree(int argc, char *argv[])
{
	pg_tree_opt_t o;
	pg_tree_opt_init(&o);
	int c;
	while ((c = getopt(argc, argv, "t:m:a:b:s:")) >= 0) {
		if (c == 't') { if ((o.type = dist_type(optarg)) < 0) { std::fprintf(stderr, "ERROR: -t must be gene or adj\n"); return 1; } }
		else if (c == 'm') { if ((o.metric = tree_metric(optarg)) < 0) { std::fprintf(stderr, "ERROR: -m must be jaccard or diff (shared is not a distance)\n"); return 1; } }
		else if (c == 'a') { if ((o.method = tree_method(optarg)) < 0) { std::fprintf(stderr, "ERROR: -a must be nj or upgma\n"); return 1; } }
		else if (c == 'b') { if (!tree_boot(optarg, o.n_boot)) { std::fprintf(stderr, "ERROR: -b must be in [0, 2147483647]\n"); return 1; } }
		else if (c == 's') { if (!tree_seed_arg(optarg, o.seed)) { std::fprintf(stderr, "ERROR: -s must be in [0, 4294967295]\n"); return 1; } }
		else return 1;
	}
	if (argc - optind < 1) {
		std::printf("Usage: pangene tree [options] <in.gfa>\nOptions:\n  -t STR   items: gene (gene content) or adj (gene adjacencies of the walks) [gene]\n"
		            "  -m STR   distance: jaccard or diff [jaccard]\n"
		            "  -a STR   nj (neighbour-joining: unrooted, negative branch lengths are printed as they come) or upgma [nj]\n"
		            "  -b INT   bootstrap replicates over the items: inner nodes are labelled with their support in per cent [0]\n"
		            "  -s INT   seed of the bootstrap draws [0]\n");
		return 0;
	}
	return pg_tree_file(argv[optind], &o) == 0 ? 0 : 1;
}

// "INT" or "INT-INT": a k or a range of k, 2 <= lo <= hi; digits only
static bool cluster_range(const char *s, int32_t &lo, int32_t &hi)
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
	lo = (int32_t)a, hi = (int32_t)b;
	return true;
}

// `pangene cluster`: k-medoids clusters of the assemblies of a GFA file over the distances `pangene dist` prints
static int main_cluster(int argc, char *argv[])
{
	pg_cluster_opt_t o;
	pg_cluster_opt_init(&o);
	bool have_k = false;
	int c;
	while ((c = getopt(argc, argv, "t:m:k:i:")) >= 0) {
		if (c == 't') { if ((o.type = dist_type(optarg)) < 0) { std::fprintf(stderr, "ERROR: -t must be gene or adj\n"); return 1; } }
		else if (c == 'm') { if ((o.metric = tree_metric(optarg)) < 0) { std::fprintf(stderr, "ERROR: -m must be jaccard or diff (shared is not a distance)\n"); return 1; } }
		else if (c == 'k') { if (!(have_k = cluster_range(optarg, o.k_lo, o.k_hi))) { std::fprintf(stderr, "ERROR: -k must be INT or INT-INT with 2 <= INT\n"); return 1; } }
		else if (c == 'i') { if (!tree_boot(optarg, o.max_iter)) { std::fprintf(stderr, "ERROR: -i must be in [0, 2147483647]\n"); return 1; } }
		else return 1;
	}
	if (argc - optind < 1) {
		std::printf("Usage: pangene cluster -k INT[-INT] [options] <in.gfa>\nOptions:\n  -k INT[-INT]  clusters: one k, or a range whose k with the largest mean silhouette is printed in full\n"
		            "  -t STR   items: gene (gene content) or adj (gene adjacencies of the walks) [gene]\n"
		            "  -m STR   distance: jaccard or diff [jaccard]\n"
		            "  -i INT   swap iterations per k at the most [1000]\n");
		return 0;
	}
	if (!have_k) { std::fprintf(stderr, "ERROR: pangene cluster needs -k INT[-INT]\n"); return 1; }
	return pg_cluster_file(argv[optind], &o) == 0 ? 0 : 1;
}

static int assoc_sign(const char *s) { return std::strcmp(s, "both") == 0 ? PG_ASSOC_BOTH : std::strcmp(s, "pos") == 0 ? PG_ASSOC_POS : std::strcmp(s, "neg") == 0 ? PG_ASSOC_NEG : -1; }
static bool assoc_phi(const char *s, double &r) // a number in [0, 1]
{
	char *e;
	r = std::strtod(s, &e);
	return e != s && *e == 0 && r >= 0.0 && r <= 1.0;
}

// `pangene assoc`: the gene pairs of a GFA file that travel together over the assemblies or exclude each other
static int main_assoc(int argc, char *argv[])
{
	pg_assoc_opt_t o;
	pg_assoc_opt_init(&o);
	int c;
	while ((c = getopt(argc, argv, "r:c:s:x:")) >= 0) {
		if (c == 'r') { if (!assoc_phi(optarg, o.min_phi)) { std::fprintf(stderr, "ERROR: -r must be in [0, 1]\n"); return 1; } }
		else if (c == 'c') { if ((o.min_count = std::atoi(optarg)) < 1) { std::fprintf(stderr, "ERROR: -c must be at least 1\n"); return 1; } }
		else if (c == 's') { if ((o.sign = assoc_sign(optarg)) < 0) { std::fprintf(stderr, "ERROR: -s must be pos, neg or both\n"); return 1; } }
		else if (c == 'x') { if ((o.max_pair = std::atoll(optarg)) < 0) { std::fprintf(stderr, "ERROR: -x must not be negative\n"); return 1; } }
		else return 1;
	}
	if (argc - optind < 1) {
		std::printf("Usage: pangene assoc [options] <in.gfa>\nOptions:\n  -r FLOAT  smallest |phi| of a reported pair, in [0, 1], read as per-mille [%g]\n"
		            "  -c INT    a gene takes part when it is present in >=INT and absent from >=INT assemblies [%d]\n"
		            "  -s STR    keep pos (co-occurring), neg (avoiding) or both [both]\n"
		            "  -x INT    give up when more than INT pairs pass [%lld]\n", o.min_phi, o.min_count, (long long)o.max_pair);
		return 0;
	}
	return pg_assoc_file(argv[optind], &o) == 0 ? 0 : 1;
}

static bool trait_perm(const char *s, int32_t &n) // an integer in [0, 2^31 - 2]
{
	char *e;
	const long long v = std::strtoll(s, &e, 10);
	if (e == s || *e != 0 || v < 0 || v > 2147483646ll) return false;
	n = (int32_t)v;
	return true;
}

static int trait_lineage(const char *s) { return std::strcmp(s, "nj") == 0 ? PG_LINEAGE_NJ : std::strcmp(s, "upgma") == 0 ? PG_LINEAGE_UPGMA : -1; }

// `pangene trait`: the association of every gene of a GFA file with the binary traits of a trait file
static int main_trait(int argc, char *argv[])
{
	pg_trait_opt_t o;
	pg_trait_opt_init(&o);
	const char *fn = nullptr;
	int c;
	while ((c = getopt(argc, argv, "t:n:s:c:p:L:")) >= 0) {
		if (c == 't') fn = optarg;
		else if (c == 'n') { if (!trait_perm(optarg, o.n_perm)) { std::fprintf(stderr, "ERROR: -n must be in [0, 2147483646]\n"); return 1; } }
		else if (c == 's') o.seed = (uint32_t)std::strtoul(optarg, nullptr, 10);
		else if (c == 'c') { if ((o.min_count = std::atoi(optarg)) < 1) { std::fprintf(stderr, "ERROR: -c must be at least 1\n"); return 1; } }
		else if (c == 'p') { char *e; o.max_p = std::strtod(optarg, &e); if (e == optarg || *e != 0 || !(o.max_p >= 0.0)) { std::fprintf(stderr, "ERROR: -p must be a number >= 0\n"); return 1; } }
		else if (c == 'L') { if ((o.lineage = trait_lineage(optarg)) < 0) { std::fprintf(stderr, "ERROR: -L must be nj or upgma\n"); return 1; } }
		else return 1;
	}
	if (argc - optind < 1) {
		std::printf("Usage: pangene trait -t FILE [options] <in.gfa>\nOptions:\n  -t FILE   traits: a header line (any first field, one name per trait), then per line an assembly and 1, 0 or NA per trait\n"
		            "  -n INT    label permutations per trait; 0: none [%d]\n  -s INT    seed of the permutations [%u]\n"
		            "  -c INT    a gene is tested when it is present in >=INT and absent from >=INT assemblies [%d]\n"
		            "  -p FLOAT  print the genes with p_fisher <= FLOAT [%g]\n"
		            "  -L STR    lineage-aware test: the pairwise comparisons on the nj or upgma tree of all assemblies (gene content, jaccard);\n"
		            "            adds the columns pairs, supp, opp, p_pair_best and p_pair_worst [none]\n", o.n_perm, o.seed, o.min_count, o.max_p);
		return 0;
	}
	if (fn == nullptr) { std::fprintf(stderr, "ERROR: pangene trait needs -t FILE\n"); return 1; }
	return pg_trait_file(argv[optind], fn, &o) == 0 ? 0 : 1;
}

// `pangene qtrait`: the rank-sum test of every gene of a GFA file against the quantitative traits of a trait file
static int main_qtrait(int argc, char *argv[])
{
	pg_qtrait_opt_t o;
	pg_qtrait_opt_init(&o);
	const char *fn = nullptr;
	int c;
	while ((c = getopt(argc, argv, "t:n:s:c:p:")) >= 0) {
		if (c == 't') fn = optarg;
		else if (c == 'n') { if (!trait_perm(optarg, o.n_perm)) { std::fprintf(stderr, "ERROR: -n must be in [0, 2147483646]\n"); return 1; } }
		else if (c == 's') o.seed = (uint32_t)std::strtoul(optarg, nullptr, 10);
		else if (c == 'c') { if ((o.min_count = std::atoi(optarg)) < 1) { std::fprintf(stderr, "ERROR: -c must be at least 1\n"); return 1; } }
		else if (c == 'p') { char *e; o.max_p = std::strtod(optarg, &e); if (e == optarg || *e != 0 || !(o.max_p >= 0.0)) { std::fprintf(stderr, "ERROR: -p must be a number >= 0\n"); return 1; } }
		else return 1;
	}
	if (argc - optind < 1) {
		std::printf("Usage: pangene qtrait -t FILE [options] <in.gfa>\nOptions:\n  -t FILE   traits: a header line (any first field, one name per trait), then per line an assembly and a number or NA per trait\n"
		            "  -n INT    permutations of the values per trait; 0: none [%d]\n  -s INT    seed of the permutations [%u]\n"
		            "  -c INT    a gene is tested when it is present in >=INT and absent from >=INT assemblies [%d]\n"
		            "  -p FLOAT  print the genes with p_wilcox <= FLOAT [%g]\n", o.n_perm, o.seed, o.min_count, o.max_p);
		return 0;
	}
	if (fn == nullptr) { std::fprintf(stderr, "ERROR: pangene qtrait needs -t FILE\n"); return 1; }
	return pg_qtrait_file(argv[optind], fn, &o) == 0 ? 0 : 1;
}

// `pangene permanova`: the two-group PERMANOVA of the assemblies' distances for every binary trait of a trait file
static int main_permanova(int argc, char *argv[])
{
	pg_permanova_opt_t o;
	pg_permanova_opt_init(&o);
	const char *fn = nullptr;
	int c;
	while ((c = getopt(argc, argv, "t:T:m:n:s:")) >= 0) {
		if (c == 't') fn = optarg;
		else if (c == 'T') { if ((o.type = dist_type(optarg)) < 0) { std::fprintf(stderr, "ERROR: -T must be gene or adj\n"); return 1; } }
		else if (c == 'm') { if ((o.metric = tree_metric(optarg)) < 0) { std::fprintf(stderr, "ERROR: -m must be jaccard or diff (shared is not a distance)\n"); return 1; } }
		else if (c == 'n') { if (!trait_perm(optarg, o.n_perm)) { std::fprintf(stderr, "ERROR: -n must be in [0, 2147483646]\n"); return 1; } }
		else if (c == 's') o.seed = (uint32_t)std::strtoul(optarg, nullptr, 10);
		else return 1;
	}
	if (argc - optind < 1) {
		std::printf("Usage: pangene permanova -t FILE [options] <in.gfa>\nOptions:\n  -t FILE   traits: a header line (any first field, one name per trait), then per line an assembly and 1, 0 or NA per trait\n"
		            "  -T STR    items: gene (gene content) or adj (gene adjacencies of the walks) [gene]\n"
		            "  -m STR    distance: jaccard or diff [jaccard]\n"
		            "  -n INT    label permutations per trait; 0: none [%d]\n  -s INT    seed of the permutations [%u]\n", o.n_perm, o.seed);
		return 0;
	}
	if (fn == nullptr) { std::fprintf(stderr, "ERROR: pangene permanova needs -t FILE\n"); return 1; }
	return pg_permanova_file(argv[optind], fn, &o) == 0 ? 0 : 1;
}

// SPEC of `pangene mantel`: gene|adj + ':' + jaccard|diff
static bool mantel_spec(const char *s, int32_t &type, int32_t &metric)
{
	const char *c = std::strchr(s, ':');
	if (c == nullptr) return false;
	const std::string t(s, c);
	const int ty = dist_type(t.c_str()), me = tree_metric(c + 1);
	if (ty < 0 || me < 0) return false;
	type = ty, metric = me;
	return true;
}

// `pangene mantel`: the Mantel test of two distance matrices of the assemblies of a GFA file, or of one of them and a matrix file
static int main_mantel(int argc, char *argv[])
{
	pg_mantel_opt_t o;
	pg_mantel_opt_init(&o);
	const char *fn = nullptr;
	bool have_y = false;
	int c;
	while ((c = getopt(argc, argv, "x:y:f:n:s:")) >= 0) {
		if (c == 'x') { if (!mantel_spec(optarg, o.x_type, o.x_metric)) { std::fprintf(stderr, "ERROR: -x must be gene|adj:jaccard|diff\n"); return 1; } }
		else if (c == 'y') { have_y = true; if (!mantel_spec(optarg, o.y_type, o.y_metric)) { std::fprintf(stderr, "ERROR: -y must be gene|adj:jaccard|diff\n"); return 1; } }
		else if (c == 'f') fn = optarg;
		else if (c == 'n') { if (!trait_perm(optarg, o.n_perm)) { std::fprintf(stderr, "ERROR: -n must be in [0, 2147483646]\n"); return 1; } }
		else if (c == 's') o.seed = (uint32_t)std::strtoul(optarg, nullptr, 10);
		else return 1;
	}
	if (argc - optind < 1) {
		std::printf("Usage: pangene mantel [options] <in.gfa>\nOptions:\n  -x SPEC   the first matrix: gene (gene content) or adj (gene adjacencies of the walks), ':', jaccard or diff [gene:jaccard]\n"
		            "  -y SPEC   the second matrix [adj:jaccard]\n"
		            "  -f FILE   the second matrix from FILE instead: the table or the PHYLIP form `pangene dist` prints\n"
		            "  -n INT    permutations of the assemblies; 0: none [%d]\n  -s INT    seed of the permutations [%u]\n", o.n_perm, o.seed);
		return 0;
	}
	if (have_y && fn != nullptr) { std::fprintf(stderr, "ERROR: -y cannot be combined with -f\n"); return 1; }
	return pg_mantel_file(argv[optind], fn, &o) == 0 ? 0 : 1;
}

static bool gainloss_cost(const char *s, int32_t &v) // an integer in [1, 255]
{
	char *e;
	const long long x = std::strtoll(s, &e, 10);
	if (e == s || *e != 0 || x < 1 || x > 255) return false;
	v = (int32_t)x;
	return true;
}
static int gainloss_mode(const char *s) { return std::strcmp(s, "late") == 0 ? PG_GAINLOSS_LATE : std::strcmp(s, "early") == 0 ? PG_GAINLOSS_EARLY : -1; }
static int gainloss_out(const char *s) { return std::strcmp(s, "gene") == 0 ? PG_GAINLOSS_GENE : std::strcmp(s, "node") == 0 ? PG_GAINLOSS_NODE : -1; }

// `pangene gainloss`: the gains and losses of every item of a GFA file on the tree `pangene tree` builds over its assemblies
static int main_gainloss(int argc, char *argv[])
{
	pg_gainloss_opt_t o;
	pg_gainloss_opt_init(&o);
	int c;
	while ((c = getopt(argc, argv, "t:m:a:g:l:r:o:c:")) >= 0) {
		if (c == 't') { if ((o.type = dist_type(optarg)) < 0) { std::fprintf(stderr, "ERROR: -t must be gene or adj\n"); return 1; } }
		else if (c == 'm') { if ((o.metric = tree_metric(optarg)) < 0) { std::fprintf(stderr, "ERROR: -m must be jaccard or diff (shared is not a distance)\n"); return 1; } }
		else if (c == 'a') { if ((o.method = tree_method(optarg)) < 0) { std::fprintf(stderr, "ERROR: -a must be upgma or nj\n"); return 1; } }
		else if (c == 'g') { if (!gainloss_cost(optarg, o.gain)) { std::fprintf(stderr, "ERROR: -g must be in [1, 255]\n"); return 1; } }
		else if (c == 'l') { if (!gainloss_cost(optarg, o.loss)) { std::fprintf(stderr, "ERROR: -l must be in [1, 255]\n"); return 1; } }
		else if (c == 'r') { if ((o.mode = gainloss_mode(optarg)) < 0) { std::fprintf(stderr, "ERROR: -r must be late or early\n"); return 1; } }
		else if (c == 'o') { if ((o.out = gainloss_out(optarg)) < 0) { std::fprintf(stderr, "ERROR: -o must be gene or node\n"); return 1; } }
		else if (c == 'c') { if (!tree_boot(optarg, o.min_changes)) { std::fprintf(stderr, "ERROR: -c must be in [0, 2147483647]\n"); return 1; } }
		else return 1;
	}
	if (argc - optind < 1) {
		std::printf("Usage: pangene gainloss [options] <in.gfa>\nOptions:\n  -t STR   items: gene (gene content) or adj (gene adjacencies of the walks) [gene]\n"
		            "  -m STR   distance of the tree: jaccard or diff [jaccard]\n"
		            "  -a STR   tree: upgma, or nj rooted at its closing join, read as ((x, y), z): gains and losses depend on that reading [upgma]\n"
		            "  -g INT   cost of a gain, 1 to 255 [%d]\n  -l INT   cost of a loss, 1 to 255 [%d]\n"
		            "  -r STR   on a tie a change sits towards the tips (late) or towards the root (early) [late]\n"
		            "  -o STR   table: gene (per item: Present Cost Changes Gains Losses Root) or node (per branch: Leaves Present Gains Losses) [gene]\n"
		            "  -c INT   -o gene: print the items with at least INT changes [%d]\n", o.gain, o.loss, o.min_changes);
		return 0;
	}
	return pg_gainloss_file(argv[optind], &o) == 0 ? 0 : 1;
}

static bool coevo_min(const char *s, int32_t &v) // an integer in [1, 2^31 - 1]
{
	char *e;
	const long long x = std::strtoll(s, &e, 10);
	if (e == s || *e != 0 || x < 1 || x > 2147483647LL) return false;
	v = (int32_t)x;
	return true;
}
static bool coevo_max(const char *s, int64_t &v) // a whole number
{
	char *e;
	const long long x = std::strtoll(s, &e, 10);
	if (e == s || *e != 0 || x < 0) return false;
	v = x;
	return true;
}

// `pangene coevo`: the item pairs of a GFA file whose gains and losses fall on the same branches of the tree `pangene tree` builds
static int main_coevo(int argc, char *argv[])
{
	pg_coevo_opt_t o;
	pg_coevo_opt_init(&o);
	int c;
	while ((c = getopt(argc, argv, "t:m:a:g:l:e:r:c:s:x:")) >= 0) {
		if (c == 't') { if ((o.type = dist_type(optarg)) < 0) { std::fprintf(stderr, "ERROR: -t must be gene or adj\n"); return 1; } }
		else if (c == 'm') { if ((o.metric = tree_metric(optarg)) < 0) { std::fprintf(stderr, "ERROR: -m must be jaccard or diff (shared is not a distance)\n"); return 1; } }
		else if (c == 'a') { if ((o.method = tree_method(optarg)) < 0) { std::fprintf(stderr, "ERROR: -a must be upgma or nj\n"); return 1; } }
		else if (c == 'g') { if (!gainloss_cost(optarg, o.gain)) { std::fprintf(stderr, "ERROR: -g must be in [1, 255]\n"); return 1; } }
		else if (c == 'l') { if (!gainloss_cost(optarg, o.loss)) { std::fprintf(stderr, "ERROR: -l must be in [1, 255]\n"); return 1; } }
		else if (c == 'e') { if ((o.mode = gainloss_mode(optarg)) < 0) { std::fprintf(stderr, "ERROR: -e must be late or early\n"); return 1; } }
		else if (c == 'r') { if (!assoc_phi(optarg, o.min_r)) { std::fprintf(stderr, "ERROR: -r must be in [0, 1]\n"); return 1; } }
		else if (c == 'c') { if (!coevo_min(optarg, o.min_events)) { std::fprintf(stderr, "ERROR: -c must be at least 1\n"); return 1; } }
		else if (c == 's') { if ((o.sign = assoc_sign(optarg)) < 0) { std::fprintf(stderr, "ERROR: -s must be pos, neg or both\n"); return 1; } }
		else if (c == 'x') { if (!coevo_max(optarg, o.max_pair)) { std::fprintf(stderr, "ERROR: -x must not be negative\n"); return 1; } }
		else return 1;
	}
	if (argc - optind < 1) {
		std::printf("Usage: pangene coevo [options] <in.gfa>\nOptions:\n  -t STR    items: gene (gene content) or adj (gene adjacencies of the walks) [gene]\n"
		            "  -m STR    distance of the tree: jaccard or diff [jaccard]\n"
		            "  -a STR    tree: upgma, or nj rooted at its closing join, read as ((x, y), z): the events depend on that reading [upgma]\n"
		            "  -g INT    cost of a gain, 1 to 255 [%d]\n  -l INT    cost of a loss, 1 to 255 [%d]\n"
		            "  -e STR    on a tie a change sits towards the tips (late) or towards the root (early) [late]\n"
		            "  -r FLOAT  smallest |r| of a reported pair, in [0, 1], read as per-mille [%g]\n"
		            "  -c INT    an item takes part with at least INT gains and losses; with 1 every pair of strain-specific genes of one assembly scores 1 [%d]\n"
		            "  -s STR    keep pos (same direction), neg (opposite direction) or both [both]\n"
		            "  -x INT    give up when more than INT pairs pass [%lld]\n", o.gain, o.loss, o.min_r, o.min_events, (long long)o.max_pair);
		return 0;
	}
	return pg_coevo_file(argv[optind], &o) == 0 ? 0 : 1;
}

// ---------------------------------------------------------------------------------------------------------------
// `pangene --gpus N`: main.c:117-142 for N devices of one node.  The command forks N - 1 workers BEFORE anything touches the GPU;
// rank r takes device r and the r-th contiguous block of the PAF files (so that the ranks' W / BED lines, concatenated in rank
// order, are in command-line order) and registers the names of the other files (ids as in a sequential read).  The exchange is
// RCCL on the kernels' stream (the 128-byte id travels through a pipe); on a backend without a device (the oracle host of the
// tests) it is a shared-memory region mapped before the fork.  Rank 0 prints the graph; every rank writes the lines of its own
// genomes to a temporary file that rank 0 copies to stdout in rank order.
// ---------------------------------------------------------------------------------------------------------------
struct Output { int matrix = 0; bool call = false; int curves = 0; uint32_t curves_seed = 11; int dist = -1, dist_metric = 0; // curves: orders (0: none); dist: PG_DIST_* (-1: none)
	bool assoc = false; double assoc_phi = 0.8; int assoc_count = 2, assoc_sign = 0;
	const char *trait = nullptr; int32_t trait_perm = 1000; uint32_t trait_seed = 11; int trait_lineage = 0;
	const char *qtrait = nullptr; int32_t qtrait_perm = 1000; uint32_t qtrait_seed = 11;
	int tree = -1, tree_metric = 0, tree_method = 0; int32_t tree_boot = 0; uint32_t tree_seed = 0; // tree: PG_DIST_GENE / PG_DIST_ADJ (-1: none)
	int32_t cluster_lo = 0, cluster_hi = 0, cluster_iter = 1000; int cluster_type = 0, cluster_metric = 0; // cluster_lo: 0 = none
	const char *permanova = nullptr; int permanova_type = 0, permanova_metric = 0; int32_t permanova_perm = 1000; uint32_t permanova_seed = 11;
	bool mantel = false; const char *mantel_file = nullptr; pg_mantel_opt_t mantel_opt;
	bool gainloss = false; pg_gainloss_opt_t gainloss_opt;
	bool coevo = false; pg_coevo_opt_t coevo_opt; };

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
		else if (o.curves) {
			pg_curves_opt_t co;
			pg_curves_opt_init(&co);
			co.n_perm = o.curves, co.seed = o.curves_seed;
			pg_write_curves(g, &co);
			if (pg_last_error()) rc = 2;
		}
		else if (o.dist >= 0) {
			pg_dist_opt_t dop;
			pg_dist_opt_init(&dop);
			dop.type = o.dist, dop.metric = o.dist_metric;
			pg_write_dist(g, &dop);
			if (pg_last_error()) rc = 2;
		}
		else if (o.assoc) {
			pg_assoc_opt_t ao;
			pg_assoc_opt_init(&ao);
			ao.min_phi = o.assoc_phi, ao.min_count = o.assoc_count, ao.sign = o.assoc_sign;
			pg_write_assoc(g, &ao);
			if (pg_last_error()) rc = 2;
		}
		else if (o.trait) {
			pg_trait_opt_t to;
			pg_trait_opt_init(&to);
			to.n_perm = o.trait_perm, to.seed = o.trait_seed, to.lineage = o.trait_lineage;
			pg_write_trait(g, o.trait, &to);
			if (pg_last_error()) rc = 2;
		}
		else if (o.qtrait) {
			pg_qtrait_opt_t qo;
			pg_qtrait_opt_init(&qo);
			qo.n_perm = o.qtrait_perm, qo.seed = o.qtrait_seed;
			pg_write_qtrait(g, o.qtrait, &qo);
			if (pg_last_error()) rc = 2;
		}
		else if (o.tree >= 0) {
			pg_tree_opt_t tro;
			pg_tree_opt_init(&tro);
			tro.type = o.tree, tro.metric = o.tree_metric, tro.method = o.tree_method, tro.n_boot = o.tree_boot, tro.seed = o.tree_seed;
			pg_write_tree(g, &tro);
			if (pg_last_error()) rc = 2;
		}
		else if (o.cluster_lo) {
			pg_cluster_opt_t clo;
			pg_cluster_opt_init(&clo);
			clo.type = o.cluster_type, clo.metric = o.cluster_metric, clo.k_lo = o.cluster_lo, clo.k_hi = o.cluster_hi, clo.max_iter = o.cluster_iter;
			pg_write_cluster(g, &clo);
			if (pg_last_error()) rc = pg_last_error() == -3 ? 1 : 2; // -3, PGA_ERR_ARG: a k outside [2, assemblies - 1] or fewer than 3 assemblies -- a refusal, as on `pangene cluster`
		}
		else if (o.permanova) {
			pg_permanova_opt_t po;
			pg_permanova_opt_init(&po);
			po.type = o.permanova_type, po.metric = o.permanova_metric, po.n_perm = o.permanova_perm, po.seed = o.permanova_seed;
			pg_write_permanova(g, o.permanova, &po);
			if (pg_last_error()) rc = 2;
		}
		else if (o.mantel) {
			pg_write_mantel(g, o.mantel_file, &o.mantel_opt);
			if (pg_last_error()) rc = 2;
		}
		else if (o.gainloss) {
			pg_write_gainloss(g, &o.gainloss_opt);
			if (pg_last_error()) rc = 2;
		}
		else if (o.coevo) {
			pg_write_coevo(g, &o.coevo_opt);
			if (pg_last_error()) rc = 2;
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
	if (o.matrix) { std::fprintf(stderr, "ERROR: --matrix needs every genome in one process; run it without --gpus\n"); return 1; }
	if (o.call) { std::fprintf(stderr, "ERROR: --call needs every genome in one process; run it without --gpus\n"); return 1; }
	if (o.curves) { std::fprintf(stderr, "ERROR: --curves needs every genome in one process; run it without --gpus\n"); return 1; }
	if (o.dist >= 0) { std::fprintf(stderr, "ERROR: --dist needs every genome in one process; run it without --gpus\n"); return 1; }
	if (o.assoc) { std::fprintf(stderr, "ERROR: --assoc needs every genome in one process; run it without --gpus\n"); return 1; }
	if (o.trait) { std::fprintf(stderr, "ERROR: --trait needs every genome in one process; run it without --gpus\n"); return 1; }
	if (o.qtrait) { std::fprintf(stderr, "ERROR: --qtrait needs every genome in one process; run it without --gpus\n"); return 1; }
	if (o.tree >= 0) { std::fprintf(stderr, "ERROR: --tree needs every genome in one process; run it without --gpus\n"); return 1; }
	if (o.cluster_lo) { std::fprintf(stderr, "ERROR: --cluster needs every genome in one process; run it without --gpus\n"); return 1; }
	if (o.permanova) { std::fprintf(stderr, "ERROR: --permanova needs every genome in one process; run it without --gpus\n"); return 1; }
	if (o.mantel) { std::fprintf(stderr, "ERROR: --mantel needs every genome in one process; run it without --gpus\n"); return 1; }
	if (o.gainloss) { std::fprintf(stderr, "ERROR: --gainloss needs every genome in one process; run it without --gpus\n"); return 1; }
	if (o.coevo) { std::fprintf(stderr, "ERROR: --coevo needs every genome in one process; run it without --gpus\n"); return 1; }
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
	if (argc >= 2 && std::strcmp(argv[1], "curves") == 0) return main_curves(argc - 1, argv + 1);
	if (argc >= 2 && std::strcmp(argv[1], "dist") == 0) return main_dist(argc - 1, argv + 1);
	if (argc >= 2 && std::strcmp(argv[1], "assoc") == 0) return main_assoc(argc - 1, argv + 1);
	if (argc >= 2 && std::strcmp(argv[1], "trait") == 0) return main_trait(argc - 1, argv + 1);
	if (argc >= 2 && std::strcmp(argv[1], "qtrait") == 0) return main_qtrait(argc - 1, argv + 1);
	if (argc >= 2 && std::strcmp(argv[1], "tree") == 0) return main_tree(argc - 1, argv + 1);
	if (argc >= 2 && std::strcmp(argv[1], "cluster") == 0) return main_cluster(argc - 1, argv + 1);
	if (argc >= 2 && std::strcmp(argv[1], "permanova") == 0) return main_permanova(argc - 1, argv + 1);
	if (argc >= 2 && std::strcmp(argv[1], "mantel") == 0) return main_mantel(argc - 1, argv + 1);
	if (argc >= 2 && std::strcmp(argv[1], "gainloss") == 0) return main_gainloss(argc - 1, argv + 1);
	if (argc >= 2 && std::strcmp(argv[1], "coevo") == 0) return main_coevo(argc - 1, argv + 1);
	int matrix = 0, n_gpus = 1; // matrix: 1 presence, 2 counts
	bool call = false;
	int curves = 0; // orders of --curves (0: not asked for)
	uint32_t curves_seed = 11;
	int dist = -1, dist_metric_v = PG_DIST_JACCARD; // --dist: PG_DIST_* (-1: not asked for)
	bool assoc = false; // --assoc
	double assoc_phi_v = 0.8;
	int assoc_count = 2, assoc_sign_v = PG_ASSOC_BOTH;
	const char *trait = nullptr; // --trait=FILE
	int32_t trait_perm_v = 1000;
	uint32_t trait_seed = 11;
	int trait_lineage_v = 0; // --trait-lineage: PG_LINEAGE_*
	const char *qtrait = nullptr; // --qtrait=FILE
	int32_t qtrait_perm_v = 1000;
	uint32_t qtrait_seed = 11;
	bool qtrait_extra = false; // a --qtrait-* option was given
	int tree = -1, tree_metric_v = PG_DIST_JACCARD, tree_method_v = PG_TREE_NJ; // --tree: PG_DIST_GENE / PG_DIST_ADJ (-1: not asked for)
	int32_t tree_boot_v = 0;
	uint32_t tree_seed = 0;
	int32_t cluster_lo = 0, cluster_hi = 0, cluster_iter_v = 1000; // --cluster: the range of k (0: not asked for)
	int cluster_type_v = PG_DIST_GENE, cluster_metric_v = PG_DIST_JACCARD;
	bool cluster_extra = false; // a --cluster-* option was given
	const char *permanova = nullptr; // --permanova=FILE
	int permanova_type_v = PG_DIST_GENE, permanova_metric_v = PG_DIST_JACCARD;
	int32_t permanova_perm_v = 1000;
	uint32_t permanova_seed = 11;
	bool permanova_extra = false; // a --permanova-* option was given
	bool mantel = false, mantel_extra = false, mantel_y = false; // --mantel[=FILE]; a --mantel-* option was given; --mantel-y was
	const char *mantel_file = nullptr;
	pg_mantel_opt_t mantel_opt;
	pg_mantel_opt_init(&mantel_opt);
	bool gainloss = false, gainloss_extra = false; // --gainloss[=gene|node]; a --gainloss-* option was given
	pg_gainloss_opt_t gainloss_opt;
	pg_gainloss_opt_init(&gainloss_opt);
	bool coevo = false, coevo_extra = false; // --coevo[=FLOAT]; a --coevo-* option was given
	pg_coevo_opt_t coevo_opt;
	pg_coevo_opt_init(&coevo_opt);
	static const struct option lopts[] = {
		{ "bed", optional_argument, nullptr, 301 }, { "ori-sc", no_argument, nullptr, 302 }, { "matrix", optional_argument, nullptr, 303 }, { "call", no_argument, nullptr, 305 },
		{ "curves", optional_argument, nullptr, 306 }, { "curves-seed", required_argument, nullptr, 307 },
		{ "dist", optional_argument, nullptr, 308 }, { "dist-metric", required_argument, nullptr, 309 },
		{ "assoc", optional_argument, nullptr, 310 }, { "assoc-min-count", required_argument, nullptr, 311 }, { "assoc-sign", required_argument, nullptr, 312 },
		{ "trait", required_argument, nullptr, 313 }, { "trait-perm", required_argument, nullptr, 314 }, { "trait-seed", required_argument, nullptr, 315 },
		{ "trait-lineage", required_argument, nullptr, 321 },
		{ "qtrait", required_argument, nullptr, 322 }, { "qtrait-perm", required_argument, nullptr, 323 }, { "qtrait-seed", required_argument, nullptr, 324 },
		{ "tree", optional_argument, nullptr, 316 }, { "tree-metric", required_argument, nullptr, 317 }, { "tree-method", required_argument, nullptr, 318 },
		{ "tree-boot", required_argument, nullptr, 319 }, { "tree-seed", required_argument, nullptr, 320 },
		{ "cluster", required_argument, nullptr, 325 }, { "cluster-type", required_argument, nullptr, 326 }, { "cluster-metric", required_argument, nullptr, 327 },
		{ "cluster-iter", required_argument, nullptr, 328 },
		{ "permanova", required_argument, nullptr, 329 }, { "permanova-type", required_argument, nullptr, 330 }, { "permanova-metric", required_argument, nullptr, 331 },
		{ "permanova-perm", required_argument, nullptr, 332 }, { "permanova-seed", required_argument, nullptr, 333 },
		{ "mantel", optional_argument, nullptr, 334 }, { "mantel-x", required_argument, nullptr, 335 }, { "mantel-y", required_argument, nullptr, 336 },
		{ "mantel-perm", required_argument, nullptr, 337 }, { "mantel-seed", required_argument, nullptr, 338 },
		{ "gainloss", optional_argument, nullptr, 339 }, { "gainloss-type", required_argument, nullptr, 340 }, { "gainloss-metric", required_argument, nullptr, 341 },
		{ "gainloss-method", required_argument, nullptr, 342 }, { "gainloss-gain", required_argument, nullptr, 343 }, { "gainloss-loss", required_argument, nullptr, 344 },
		{ "gainloss-resolve", required_argument, nullptr, 345 }, { "gainloss-min", required_argument, nullptr, 346 },
		{ "coevo", optional_argument, nullptr, 347 }, { "coevo-type", required_argument, nullptr, 348 }, { "coevo-metric", required_argument, nullptr, 349 },
		{ "coevo-method", required_argument, nullptr, 350 }, { "coevo-gain", required_argument, nullptr, 351 }, { "coevo-loss", required_argument, nullptr, 352 },
		{ "coevo-resolve", required_argument, nullptr, 353 }, { "coevo-min", required_argument, nullptr, 354 }, { "coevo-sign", required_argument, nullptr, 355 },
		{ "coevo-max", required_argument, nullptr, 356 },
		{ "gpus", required_argument, nullptr, 304 }, { "procs", required_argument, nullptr, 304 },
		{ "version", no_argument, nullptr, 401 }, { nullptr, 0, nullptr, 0 } };
	pg_opt_t opt;
	pg_opt_init(&opt);
	int c;
	while ((c = getopt_long(argc, argv, "d:e:l:f:g:p:b:B:y:Fr:c:a:wv:GD:C:T:X:I:P:m:JOSE", lopts, nullptr)) >= 0) {
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
		case 303: matrix = (optarg && std::strcmp(optarg, "count") == 0) ? 2 : 1; break;
		case 304: n_gpus = std::atoi(optarg); break;
		case 305: call = true; break;
		case 306:
			curves = optarg ? std::atoi(optarg) : 10;
			if (curves < 1) { std::fprintf(stderr, "ERROR: --curves needs at least one order\n"); return 1; }
			break;
		case 307: curves_seed = (uint32_t)std::strtoul(optarg, nullptr, 10); break;
		case 308:
			dist = optarg ? dist_type(optarg) : PG_DIST_GENE;
			if (dist < 0) { std::fprintf(stderr, "ERROR: --dist must be gene or adj\n"); return 1; }
			break;
		case 309:
			dist_metric_v = dist_metric(optarg);
			if (dist_metric_v < 0) { std::fprintf(stderr, "ERROR: --dist-metric must be jaccard, shared or diff\n"); return 1; }
			break;
		case 310:
			assoc = true;
			if (optarg && !assoc_phi(optarg, assoc_phi_v)) { std::fprintf(stderr, "ERROR: --assoc must be in [0, 1]\n"); return 1; }
			break;
		case 311:
			if ((assoc_count = std::atoi(optarg)) < 1) { std::fprintf(stderr, "ERROR: --assoc-min-count must be at least 1\n"); return 1; }
			break;
		case 312:
			if ((assoc_sign_v = assoc_sign(optarg)) < 0) { std::fprintf(stderr, "ERROR: --assoc-sign must be pos, neg or both\n"); return 1; }
			break;
		case 313: trait = optarg; break;
		case 314:
			if (!trait_perm(optarg, trait_perm_v)) { std::fprintf(stderr, "ERROR: --trait-perm must be in [0, 2147483646]\n"); return 1; }
			break;
		case 315: trait_seed = (uint32_t)std::strtoul(optarg, nullptr, 10); break;
		case 316:
			tree = optarg ? dist_type(optarg) : PG_DIST_GENE;
			if (tree < 0) { std::fprintf(stderr, "ERROR: --tree must be gene or adj\n"); return 1; }
			break;
		case 317:
			if ((tree_metric_v = tree_metric(optarg)) < 0) { std::fprintf(stderr, "ERROR: --tree-metric must be jaccard or diff (shared is not a distance)\n"); return 1; }
			break;
		case 318:
			if ((tree_method_v = tree_method(optarg)) < 0) { std::fprintf(stderr, "ERROR: --tree-method must be nj or upgma\n"); return 1; }
			break;
		case 319:
			if (!tree_boot(optarg, tree_boot_v)) { std::fprintf(stderr, "ERROR: --tree-boot must be in [0, 2147483647]\n"); return 1; }
			break;
		case 320:
			if (!tree_seed_arg(optarg, tree_seed)) { std::fprintf(stderr, "ERROR: --tree-seed must be in [0, 4294967295]\n"); return 1; }
			break;
		case 321:
			if ((trait_lineage_v = trait_lineage(optarg)) < 0) { std::fprintf(stderr, "ERROR: --trait-lineage must be nj or upgma\n"); return 1; }
			break;
		case 322: qtrait = optarg; break;
		case 323:
			qtrait_extra = true;
			if (!trait_perm(optarg, qtrait_perm_v)) { std::fprintf(stderr, "ERROR: --qtrait-perm must be in [0, 2147483646]\n"); return 1; }
			break;
		case 324: qtrait_extra = true, qtrait_seed = (uint32_t)std::strtoul(optarg, nullptr, 10); break;
		case 325:
			if (!cluster_range(optarg, cluster_lo, cluster_hi)) { std::fprintf(stderr, "ERROR: --cluster must be INT or INT-INT with 2 <= INT\n"); return 1; }
			break;
		case 326:
			cluster_extra = true;
			if ((cluster_type_v = dist_type(optarg)) < 0) { std::fprintf(stderr, "ERROR: --cluster-type must be gene or adj\n"); return 1; }
			break;
		case 327:
			cluster_extra = true;
			if ((cluster_metric_v = tree_metric(optarg)) < 0) { std::fprintf(stderr, "ERROR: --cluster-metric must be jaccard or diff (shared is not a distance)\n"); return 1; }
			break;
		case 328:
			cluster_extra = true;
			if (!tree_boot(optarg, cluster_iter_v)) { std::fprintf(stderr, "ERROR: --cluster-iter must be in [0, 2147483647]\n"); return 1; }
			break;
		case 329: permanova = optarg; break;
		case 330:
			permanova_extra = true;
			if ((permanova_type_v = dist_type(optarg)) < 0) { std::fprintf(stderr, "ERROR: --permanova-type must be gene or adj\n"); return 1; }
			break;
		case 331:
			permanova_extra = true;
			if ((permanova_metric_v = tree_metric(optarg)) < 0) { std::fprintf(stderr, "ERROR: --permanova-metric must be jaccard or diff (shared is not a distance)\n"); return 1; }
			break;
		case 332:
			permanova_extra = true;
			if (!trait_perm(optarg, permanova_perm_v)) { std::fprintf(stderr, "ERROR: --permanova-perm must be in [0, 2147483646]\n"); return 1; }
			break;
		case 333: permanova_extra = true, permanova_seed = (uint32_t)std::strtoul(optarg, nullptr, 10); break;
		case 334: mantel = true, mantel_file = optarg; break;
		case 335:
			mantel_extra = true;
			if (!mantel_spec(optarg, mantel_opt.x_type, mantel_opt.x_metric)) { std::fprintf(stderr, "ERROR: --mantel-x must be gene|adj:jaccard|diff\n"); return 1; }
			break;
		case 336:
			mantel_extra = mantel_y = true;
			if (!mantel_spec(optarg, mantel_opt.y_type, mantel_opt.y_metric)) { std::fprintf(stderr, "ERROR: --mantel-y must be gene|adj:jaccard|diff\n"); return 1; }
			break;
		case 337:
			mantel_extra = true;
			if (!trait_perm(optarg, mantel_opt.n_perm)) { std::fprintf(stderr, "ERROR: --mantel-perm must be in [0, 2147483646]\n"); return 1; }
			break;
		case 338: mantel_extra = true, mantel_opt.seed = (uint32_t)std::strtoul(optarg, nullptr, 10); break;
		case 339:
			gainloss = true;
			if (optarg && (gainloss_opt.out = gainloss_out(optarg)) < 0) { std::fprintf(stderr, "ERROR: --gainloss must be gene or node\n"); return 1; }
			break;
		case 340:
			gainloss_extra = true;
			if ((gainloss_opt.type = dist_type(optarg)) < 0) { std::fprintf(stderr, "ERROR: --gainloss-type must be gene or adj\n"); return 1; }
			break;
		case 341:
			gainloss_extra = true;
			if ((gainloss_opt.metric = tree_metric(optarg)) < 0) { std::fprintf(stderr, "ERROR: --gainloss-metric must be jaccard or diff (shared is not a distance)\n"); return 1; }
			break;
		case 342:
			gainloss_extra = true;
			if ((gainloss_opt.method = tree_method(optarg)) < 0) { std::fprintf(stderr, "ERROR: --gainloss-method must be upgma or nj\n"); return 1; }
			break;
		case 343:
			gainloss_extra = true;
			if (!gainloss_cost(optarg, gainloss_opt.gain)) { std::fprintf(stderr, "ERROR: --gainloss-gain must be in [1, 255]\n"); return 1; }
			break;
		case 344:
			gainloss_extra = true;
			if (!gainloss_cost(optarg, gainloss_opt.loss)) { std::fprintf(stderr, "ERROR: --gainloss-loss must be in [1, 255]\n"); return 1; }
			break;
		case 345:
			gainloss_extra = true;
			if ((gainloss_opt.mode = gainloss_mode(optarg)) < 0) { std::fprintf(stderr, "ERROR: --gainloss-resolve must be late or early\n"); return 1; }
			break;
		case 346:
			gainloss_extra = true;
			if (!tree_boot(optarg, gainloss_opt.min_changes)) { std::fprintf(stderr, "ERROR: --gainloss-min must be in [0, 2147483647]\n"); return 1; }
			break;
		case 347:
			coevo = true;
			if (optarg && !assoc_phi(optarg, coevo_opt.min_r)) { std::fprintf(stderr, "ERROR: --coevo must be in [0, 1]\n"); return 1; }
			break;
		case 348:
			coevo_extra = true;
			if ((coevo_opt.type = dist_type(optarg)) < 0) { std::fprintf(stderr, "ERROR: --coevo-type must be gene or adj\n"); return 1; }
			break;
		case 349:
			coevo_extra = true;
			if ((coevo_opt.metric = tree_metric(optarg)) < 0) { std::fprintf(stderr, "ERROR: --coevo-metric must be jaccard or diff (shared is not a distance)\n"); return 1; }
			break;
		case 350:
			coevo_extra = true;
			if ((coevo_opt.method = tree_method(optarg)) < 0) { std::fprintf(stderr, "ERROR: --coevo-method must be upgma or nj\n"); return 1; }
			break;
		case 351:
			coevo_extra = true;
			if (!gainloss_cost(optarg, coevo_opt.gain)) { std::fprintf(stderr, "ERROR: --coevo-gain must be in [1, 255]\n"); return 1; }
			break;
		case 352:
			coevo_extra = true;
			if (!gainloss_cost(optarg, coevo_opt.loss)) { std::fprintf(stderr, "ERROR: --coevo-loss must be in [1, 255]\n"); return 1; }
			break;
		case 353:
			coevo_extra = true;
			if ((coevo_opt.mode = gainloss_mode(optarg)) < 0) { std::fprintf(stderr, "ERROR: --coevo-resolve must be late or early\n"); return 1; }
			break;
		case 354:
			coevo_extra = true;
			if (!coevo_min(optarg, coevo_opt.min_events)) { std::fprintf(stderr, "ERROR: --coevo-min must be at least 1\n"); return 1; }
			break;
		case 355:
			coevo_extra = true;
			if ((coevo_opt.sign = assoc_sign(optarg)) < 0) { std::fprintf(stderr, "ERROR: --coevo-sign must be pos, neg or both\n"); return 1; }
			break;
		case 356:
			coevo_extra = true;
			if (!coevo_max(optarg, coevo_opt.max_pair)) { std::fprintf(stderr, "ERROR: --coevo-max must not be negative\n"); return 1; }
			break;
		case 401: std::puts(PG_VERSION); return 0;
		default: break;
		}
	}
	if (argc - optind < 1) return usage(stderr, &opt);
	if (curves && (matrix || call)) { std::fprintf(stderr, "ERROR: --curves cannot be combined with --matrix or --call\n"); return 1; }
	if (dist >= 0 && (matrix || call || curves)) { std::fprintf(stderr, "ERROR: --dist cannot be combined with --matrix, --call or --curves\n"); return 1; }
	if (assoc && (matrix || call || curves || dist >= 0)) { std::fprintf(stderr, "ERROR: --assoc cannot be combined with --matrix, --call, --curves or --dist\n"); return 1; }
	if (trait && (matrix || call || curves || dist >= 0 || assoc)) { std::fprintf(stderr, "ERROR: --trait cannot be combined with --matrix, --call, --curves, --dist or --assoc\n"); return 1; }
	if (trait_lineage_v && !trait) { std::fprintf(stderr, "ERROR: --trait-lineage needs --trait=FILE\n"); return 1; }
	if (tree >= 0 && (matrix || call || curves || dist >= 0 || assoc || trait)) { std::fprintf(stderr, "ERROR: --tree cannot be combined with --matrix, --call, --curves, --dist, --assoc or --trait\n"); return 1; }
	if (qtrait && (matrix || call || curves || dist >= 0 || assoc || trait || tree >= 0)) { std::fprintf(stderr, "ERROR: --qtrait cannot be combined with --matrix, --call, --curves, --dist, --assoc, --trait or --tree\n"); return 1; }
	if (qtrait_extra && !qtrait) { std::fprintf(stderr, "ERROR: --qtrait-perm and --qtrait-seed need --qtrait=FILE\n"); return 1; }
	if (cluster_lo && (matrix || call || curves || dist >= 0 || assoc || trait || tree >= 0 || qtrait)) {
		std::fprintf(stderr, "ERROR: --cluster cannot be combined with --matrix, --call, --curves, --dist, --assoc, --trait, --tree or --qtrait\n");
		return 1;
	}
	if (cluster_extra && !cluster_lo) { std::fprintf(stderr, "ERROR: --cluster-type, --cluster-metric and --cluster-iter need --cluster=INT[-INT]\n"); return 1; }
	if (permanova && (matrix || call || curves || dist >= 0 || assoc || trait || tree >= 0 || qtrait || cluster_lo)) {
		std::fprintf(stderr, "ERROR: --permanova cannot be combined with --matrix, --call, --curves, --dist, --assoc, --trait, --tree, --qtrait or --cluster\n");
		return 1;
	}
	if (permanova_extra && !permanova) { std::fprintf(stderr, "ERROR: --permanova-type, --permanova-metric, --permanova-perm and --permanova-seed need --permanova=FILE\n"); return 1; }
	if (mantel && (matrix || call || curves || dist >= 0 || assoc || trait || tree >= 0 || qtrait || cluster_lo || permanova)) {
		std::fprintf(stderr, "ERROR: --mantel cannot be combined with --matrix, --call, --curves, --dist, --assoc, --trait, --tree, --qtrait, --cluster or --permanova\n");
		return 1;
	}
	if (mantel_extra && !mantel) { std::fprintf(stderr, "ERROR: --mantel-x, --mantel-y, --mantel-perm and --mantel-seed need --mantel\n"); return 1; }
	if (mantel_y && mantel_file) { std::fprintf(stderr, "ERROR: --mantel-y cannot be combined with --mantel=FILE\n"); return 1; }
	if (gainloss && (matrix || call || curves || dist >= 0 || assoc || trait || tree >= 0 || qtrait || cluster_lo || permanova || mantel)) {
		std::fprintf(stderr, "ERROR: --gainloss cannot be combined with --matrix, --call, --curves, --dist, --assoc, --trait, --tree, --qtrait, --cluster, --permanova or --mantel\n");
		return 1;
	}
	if (gainloss_extra && !gainloss) {
		std::fprintf(stderr, "ERROR: --gainloss-type, --gainloss-metric, --gainloss-method, --gainloss-gain, --gainloss-loss, --gainloss-resolve and --gainloss-min need --gainloss\n");
		return 1;
	}
	if (coevo && (matrix || call || curves || dist >= 0 || assoc || trait || tree >= 0 || qtrait || cluster_lo || permanova || mantel || gainloss)) {
		std::fprintf(stderr, "ERROR: --coevo cannot be combined with --matrix, --call, --curves, --dist, --assoc, --trait, --tree, --qtrait, --cluster, --permanova, --mantel or --gainloss\n");
		return 1;
	}
	if (coevo_extra && !coevo) {
		std::fprintf(stderr, "ERROR: --coevo-type, --coevo-metric, --coevo-method, --coevo-gain, --coevo-loss, --coevo-resolve, --coevo-min, --coevo-sign and --coevo-max need --coevo\n");
		return 1;
	}
	Output o;
	o.coevo = coevo, o.coevo_opt = coevo_opt;
	o.gainloss = gainloss, o.gainloss_opt = gainloss_opt;
	o.mantel = mantel, o.mantel_file = mantel_file, o.mantel_opt = mantel_opt;
	o.permanova = permanova, o.permanova_type = permanova_type_v, o.permanova_metric = permanova_metric_v, o.permanova_perm = permanova_perm_v, o.permanova_seed = permanova_seed;
	o.cluster_lo = cluster_lo, o.cluster_hi = cluster_hi, o.cluster_iter = cluster_iter_v, o.cluster_type = cluster_type_v, o.cluster_metric = cluster_metric_v;
	o.qtrait = qtrait, o.qtrait_perm = qtrait_perm_v, o.qtrait_seed = qtrait_seed;
	o.tree = tree, o.tree_metric = tree_metric_v, o.tree_method = tree_method_v, o.tree_boot = tree_boot_v, o.tree_seed = tree_seed;
	o.trait = trait, o.trait_perm = trait_perm_v, o.trait_seed = trait_seed, o.trait_lineage = trait_lineage_v;
	o.assoc = assoc, o.assoc_phi = assoc_phi_v, o.assoc_count = assoc_count, o.assoc_sign = assoc_sign_v;
	o.curves = curves, o.curves_seed = curves_seed;
	o.dist = dist, o.dist_metric = dist_metric_v;
	o.matrix = matrix;
	o.call = call;
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
