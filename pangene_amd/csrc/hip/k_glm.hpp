// ------------------------------------------------------------------------------------------------
// Structure-adjusted association (pga_pan_glm; DESIGN.md section 8 "Structure-adjusted association"): the Rao score test of every gene
// against every trait, given the null fit the host made.  Per trait the host hands over 16 doubles an assembly -- valid, r, w,
// w z_1 .. w z_13, a whole row of zeros for an assembly without a value -- and the Cholesky factor L of Z'WZ.  The per-gene work is one
// row of the product S = X . cols of the presence BITS with those columns, then a forward substitution:
//   sums   k_glm_sums: S on v_mfma_f64_16x16x4_f64, the fp64 matrix cores.  One MFMA tile is 16 genes x the 16 columns of one trait over
//          4 assemblies.  A operand: lane l holds the bit of gene l & 15 at assembly c0 + (l >> 4) as 0.0 or 1.0, made from the 32-bit
//          word the lane loaded for 32 assemblies (eight steps a word); the bit matrix stays the only copy of the presence data in HBM.
//          B operand: lane l holds cols[c0 + (l >> 4)][l & 15], i.e. double number l of the step's 512 contiguous bytes.  A workgroup
//          is four waves, a wave has GLM_TILES = 4 gene tiles (four independent accumulators), so 256 genes share one staged chunk of
//          GLM_KC = 128 assemblies x 16 columns (16 KiB of LDS, read without bank conflicts: lane l reads double l): the columns are
//          read from L2 once per 256 genes.  The traits are grid.y.
//          THE RESULT MAP of the f64 MFMA is not the one the other 16 x 16 MFMAs have: column = l & 15, row = (l >> 4) + 4 register
//          (not 4 (l >> 4) + register).
//          Where genes x traits leave the chip empty the sum over the assemblies is split into grid.z segments of whole chunks; every
//          segment writes its own partial S, and k_glm_stat adds the partials in ascending order of the segment.  No float atomics: the
//          same call returns the same bits.
//   stat   k_glm_stat: one lane per (trait, gene), L in LDS.  a = S_0 (an exact integer), U = S_1, s_w = S_2, b = (S_2 .. S_{2+k}),
//          y = L^-1 b by forward substitution in ascending order, V = s_w - |y|^2.  Four values a gene go back to the host.
// ------------------------------------------------------------------------------------------------
constexpr int32_t GLM_COLS = 16;                            // doubles of an assembly's row of one trait
constexpr int32_t GLM_MAX_COV = 13;                         // covariates beside the intercept: columns 3 .. 15
constexpr int32_t GLM_KC = 128;                             // assemblies of a staged chunk: four words, 32 MFMA steps
constexpr int32_t GLM_TILES = 4;                            // gene tiles of a wave
constexpr int32_t GLM_GENES = BLOCK / WAVE * GLM_TILES * 16; // genes of a workgroup: 256

typedef double glm_v4d __attribute__((ext_vector_type(4)));

// grid: (ceil(G / 256), T, n_seg).  bits[G][W]; cols[T][a_pad][16] with a_pad a multiple of GLM_KC and zero rows past the assemblies;
// segment z sums the chunks [z cps, min((z + 1) cps, a_pad / GLM_KC)) -- never an empty range -- into part[z][T][G][16].
__global__ __launch_bounds__(BLOCK) void k_glm_sums(const uint32_t *__restrict__ bits, const double *__restrict__ cols, int32_t G, int32_t W, int32_t a_pad, int32_t cps,
                                                    double *__restrict__ part)
{
	__shared__ double sh[GLM_KC * GLM_COLS];
	const int32_t t = (int32_t)threadIdx.x, lane = t & (WAVE - 1), wv = t / WAVE;
	const int32_t fr = lane & 15, fk = lane >> 4; // operand fragment: gene / column, assembly of the step
	const int32_t trait = (int32_t)blockIdx.y, n_trait = (int32_t)gridDim.y, seg = (int32_t)blockIdx.z;
	const int32_t g0 = (int32_t)blockIdx.x * GLM_GENES + wv * (GLM_TILES * 16);
	const int32_t n_chunk = a_pad / GLM_KC, c_lo = seg * cps, c_hi = min(n_chunk, c_lo + cps);

	glm_v4d acc[GLM_TILES];
	const uint32_t *row[GLM_TILES];
	bool ok[GLM_TILES];
#pragma unroll
	for (int32_t m = 0; m < GLM_TILES; ++m) {
		acc[m] = glm_v4d{0.0, 0.0, 0.0, 0.0};
		ok[m] = g0 + 16 * m + fr < G;
		row[m] = bits + (size_t)(ok[m] ? g0 + 16 * m + fr : 0) * (size_t)W;
	}
	const double *cbase = cols + (size_t)trait * (size_t)a_pad * GLM_COLS;
	for (int32_t c = c_lo; c < c_hi; ++c) {
		const double2 *src = (const double2 *)(cbase + (size_t)c * (GLM_KC * GLM_COLS));
#pragma unroll
		for (int32_t q = 0; q < GLM_KC * GLM_COLS / 2 / BLOCK; ++q) ((double2 *)sh)[t + BLOCK * q] = src[t + BLOCK * q];
		uint32_t w[GLM_TILES][GLM_KC / 32];
#pragma unroll
		for (int32_t m = 0; m < GLM_TILES; ++m)
#pragma unroll
			for (int32_t j = 0; j < GLM_KC / 32; ++j) {
				const int32_t wi = c * (GLM_KC / 32) + j;
				w[m][j] = ok[m] && wi < W ? row[m][wi] : 0u;
			}
		__syncthreads();
#pragma unroll
		for (int32_t j = 0; j < GLM_KC / 32; ++j)
#pragma unroll
			for (int32_t s = 0; s < 8; ++s) {
				const double b = sh[j * (32 * GLM_COLS) + s * WAVE + lane]; // cols[32 j + 4 s + fk][fr]
#pragma unroll
				for (int32_t m = 0; m < GLM_TILES; ++m) {
					const double a = __hiloint2double((w[m][j] >> (4 * s + fk)) & 1u ? 0x3FF00000 : 0, 0); // 1.0 or 0.0
					acc[m] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[m], 0, 0, 0);
				}
			}
		__syncthreads();
	}
	// the f64 result map: register r of tile m is gene g0 + 16 m + fk + 4 r, column fr
#pragma unroll
	for (int32_t m = 0; m < GLM_TILES; ++m)
#pragma unroll
		for (int32_t r = 0; r < 4; ++r) {
			const int32_t g = g0 + 16 * m + fk + 4 * r;
			if (g < G) part[(((size_t)seg * (size_t)n_trait + (size_t)trait) * (size_t)G + (size_t)g) * GLM_COLS + (size_t)fr] = acc[m][r];
		}
}

// grid: (ceil(G / 256), T).  part[n_seg][T][G][16], chol[T][k1][k1] (row-major, lower triangle); a, u, v, sw[T][G]; sums: NULL, or (tests)
// sums[T][G][16] = S.
__global__ __launch_bounds__(BLOCK) void k_glm_stat(const double *__restrict__ part, const double *__restrict__ chol, int32_t G, int32_t n_seg, int32_t k1,
                                                    int32_t *__restrict__ a_out, double *__restrict__ u_out, double *__restrict__ v_out, double *__restrict__ sw_out,
                                                    double *__restrict__ sums)
{
	__shared__ double L[(GLM_MAX_COV + 1) * (GLM_MAX_COV + 1)];
	const int32_t t = (int32_t)threadIdx.x, trait = (int32_t)blockIdx.y, n_trait = (int32_t)gridDim.y;
	for (int32_t i = t; i < k1 * k1; i += BLOCK) L[i] = chol[(size_t)trait * (size_t)(k1 * k1) + (size_t)i];
	__syncthreads();
	const int32_t g = (int32_t)blockIdx.x * BLOCK + t;
	if (g >= G) return;
	double S[GLM_COLS];
#pragma unroll
	for (int32_t c = 0; c < GLM_COLS; ++c) S[c] = 0.0;
	for (int32_t s = 0; s < n_seg; ++s) { // ascending: the one order
		const double2 *p = (const double2 *)(part + (((size_t)s * (size_t)n_trait + (size_t)trait) * (size_t)G + (size_t)g) * GLM_COLS);
#pragma unroll
		for (int32_t c = 0; c < GLM_COLS / 2; ++c) { const double2 x = p[c]; S[2 * c] += x.x, S[2 * c + 1] += x.y; }
	}
	const size_t at = (size_t)trait * (size_t)G + (size_t)g;
	if (sums != nullptr) {
#pragma unroll
		for (int32_t c = 0; c < GLM_COLS; ++c) sums[at * GLM_COLS + c] = S[c];
	}
	double y[GLM_MAX_COV + 1], q = 0.0;
#pragma unroll
	for (int32_t i = 0; i <= GLM_MAX_COV; ++i) {
		y[i] = 0.0;
		if (i < k1) {
			double b = S[2 + i];
#pragma unroll
			for (int32_t j = 0; j < i; ++j) b -= L[i * k1 + j] * y[j];
			y[i] = b / L[i * k1 + i];
			q += y[i] * y[i];
		}
	}
	a_out[at] = (int32_t)S[0], u_out[at] = S[1], sw_out[at] = S[2], v_out[at] = S[2] - q;
}
