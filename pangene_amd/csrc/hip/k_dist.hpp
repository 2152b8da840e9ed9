// ------------------------------------------------------------------------------------------------
// Pairwise shared items (pga_pan_shared): S[i][j] = popcount(B_i & B_j) over the assemblies' bit rows, an all-pairs Gram matrix
// over bits.  One workgroup per 128 x 128 output tile of the upper triangle (ti <= tj; the 1-D grid is mapped to (ti, tj)), and
// where there are too few tiles to fill the device, per slice of the K chunks as well (n_split > 1: the slices add into S, which the
// host zeroed).  Per 32-word K chunk the two row blocks are staged in LDS (36 KiB; 220 VGPRs allow two workgroups per CU, and one's
// loads hide behind the other's compute); each of the 256 threads keeps an 8 x 8 micro-tile, rows ty + 16 ii and columns tx + 16 jj, and
// adds popc(a & b) for every word pair: v_and_b32 + v_bcnt_u32_b32 with the accumulator as its second operand, 2 VALU ops per pair
// (an empty asm after each add keeps the compiler from regrouping the four adds of a 16-byte read into v_add3_u32 trees, 2.5 ops
// per pair).  LDS rows are 36 words apart, so the 16 rows a ds_read_b128 lane group reads fall on 16 distinct 4-bank slots.  The
// finished tile goes through LDS once more, 64 rows at a time, so that it and its mirror are both written as whole 512-byte rows.
// ------------------------------------------------------------------------------------------------
constexpr int32_t DIST_TILE = 128;                        // output tile edge
constexpr int32_t DIST_KC = 32;                           // words per K chunk
constexpr int32_t DIST_LDW = DIST_KC + 4;                 // LDS row stride in words
constexpr int32_t DIST_SIDE = DIST_TILE * DIST_LDW;       // words of one staged row block
constexpr int32_t DIST_OUTW = DIST_TILE + 1;              // LDS row stride of the finished tile
constexpr int32_t DIST_LDS_WORDS = 2 * DIST_SIDE;         // the two row blocks: 36 864 B
constexpr int32_t DIST_LOADS = 2 * DIST_TILE * DIST_KC / BLOCK; // words each thread stages per chunk (both row blocks)
static_assert(DIST_TILE / 2 * DIST_OUTW <= DIST_LDS_WORDS, "half the finished tile reuses the staging buffer");
static_assert(BLOCK == 256, "16 x 16 threads of 8 x 8 each");

// The tile body k_dist_shared, k_assoc_pairs (k_assoc.hpp) and k_trait_count (k_trait.hpp) share: acc[ii][jj] = sum over the words of
// chunks [c_lo, c_hi) of popc(ra[i0 + ty + 16 ii][.] & rb[j0 + tx + 16 jj][.]), rows past na / nb and words past W counting as zero.
// trim: the inner loop stops at the last word of the rows (the words past W are staged as zeros either way).  It is a macro and not a
// __forceinline__ function because the compiler optimises such a function on its own before it inlines it, and what comes out differs
// from the body written in the kernel (other address arithmetic in the staging, other register counts), while the numbers of DESIGN
// section 8 were measured on exactly this code.  Expanded in the kernel's scope, it uses the kernel's t, tx, ty (thread, column and
// row of the 16 x 16 layout), i0, j0 (first rows of the tile), sh (DIST_LDS_WORDS words of LDS, 16-byte aligned) and declares and fills
// uint32_t acc[8][8].  The kernel may use sh again after a __syncthreads().
#define BIT_TILE(trim, ra, na, rb, nb, W, c_lo, c_hi) \
	uint32_t acc[8][8]; \
	_Pragma("unroll") for (int32_t ii = 0; ii < 8; ++ii) \
		_Pragma("unroll") for (int32_t jj = 0; jj < 8; ++jj) acc[ii][jj] = 0; \
	const uint32_t *sa = sh, *sb = sh + DIST_SIDE; \
	for (int32_t c = (c_lo); c < (c_hi); ++c) { \
		/* row block i, then row block j: word e = t + BLOCK * r of the block's chunk at row e >> 5, word e & 31, so 32 lanes read one */ \
		/* 128-byte row piece */ \
		_Pragma("unroll") for (int32_t side = 0; side < 2; ++side) { \
			uint32_t v[DIST_LOADS / 2]; \
			const int32_t g0 = side ? j0 : i0, n_row = side ? (nb) : (na); \
			const uint32_t *src = side ? (rb) : (ra); \
			_Pragma("unroll") for (int32_t r = 0; r < DIST_LOADS / 2; ++r) { \
				const int32_t e = t + BLOCK * r, g = g0 + (e >> 5), k = c * DIST_KC + (e & 31); \
				v[r] = (g < n_row && k < (W)) ? src[(size_t)g * (size_t)(W) + (size_t)k] : 0u; \
			} \
			if (side == 0 && c > (c_lo)) __syncthreads(); /* everyone is done with the previous chunk */ \
			_Pragma("unroll") for (int32_t r = 0; r < DIST_LOADS / 2; ++r) { \
				const int32_t e = t + BLOCK * r; \
				sh[side * DIST_SIDE + (e >> 5) * DIST_LDW + (e & 31)] = v[r]; \
			} \
		} \
		__syncthreads(); \
		const int32_t kk_hi = (trim) ? min(DIST_KC, ((W) - c * DIST_KC + 3) & ~3) : DIST_KC; \
		_Pragma("unroll 1") for (int32_t kk = 0; kk < kk_hi; kk += 4) { \
			uint4 a[8], b[8]; \
			_Pragma("unroll") for (int32_t ii = 0; ii < 8; ++ii) a[ii] = *(const uint4 *)(sa + (ty + 16 * ii) * DIST_LDW + kk); \
			_Pragma("unroll") for (int32_t jj = 0; jj < 8; ++jj) b[jj] = *(const uint4 *)(sb + (tx + 16 * jj) * DIST_LDW + kk); \
			_Pragma("unroll") for (int32_t ii = 0; ii < 8; ++ii) \
				_Pragma("unroll") for (int32_t jj = 0; jj < 8; ++jj) { \
					uint32_t x = acc[ii][jj]; \
					x = __popc(a[ii].x & b[jj].x) + x; asm volatile("" : "+v"(x)); \
					x = __popc(a[ii].y & b[jj].y) + x; asm volatile("" : "+v"(x)); \
					x = __popc(a[ii].z & b[jj].z) + x; asm volatile("" : "+v"(x)); \
					x = __popc(a[ii].w & b[jj].w) + x; asm volatile("" : "+v"(x)); \
					acc[ii][jj] = x; \
				} \
		} \
	}

// the upper-triangle tile q = tj (tj + 1) / 2 + ti, ti <= tj
__device__ __forceinline__ void dist_tile_of(int32_t q, int32_t &ti, int32_t &tj)
{
	int32_t j = (int32_t)((sqrt(8.0 * (double)q + 1.0) - 1.0) * 0.5);
	while (j > 0 && j * (j + 1) / 2 > q) --j;
	while ((j + 1) * (j + 2) / 2 <= q) ++j;
	tj = j, ti = q - j * (j + 1) / 2;
}

// grid: n_tile * n_split blocks; slice sp of a tile takes chunks [sp * cps, min(n_chunk, (sp + 1) * cps))
__global__ __launch_bounds__(BLOCK, 2) void k_dist_shared(const uint32_t *__restrict__ bits, int32_t A, int32_t W, int32_t n_chunk,
                                                         int32_t n_split, int32_t cps, int32_t *__restrict__ S)
{
	__shared__ uint4 sh4[DIST_LDS_WORDS / 4];
	uint32_t *sh = (uint32_t *)sh4;
	const int32_t t = (int32_t)threadIdx.x, tx = t & 15, ty = t >> 4;
	const int32_t q = (int32_t)(blockIdx.x / (uint32_t)n_split), sp = (int32_t)(blockIdx.x % (uint32_t)n_split);
	int32_t ti, tj;
	dist_tile_of(q, ti, tj);
	const int32_t i0 = ti * DIST_TILE, j0 = tj * DIST_TILE;
	const int32_t c_lo = sp * cps, c_hi = min(n_chunk, c_lo + cps);

	BIT_TILE(false, bits, A, bits, A, W, c_lo, c_hi)

	// the finished tile through LDS, rows h * 64 .. h * 64 + 63 at a time; row-wise stores of the tile and (off the diagonal) its mirror
	int32_t *st = (int32_t *)sh;
	const bool add = n_split > 1;
	const size_t An = (size_t)A;
#pragma unroll
	for (int32_t h = 0; h < 2; ++h) {
		__syncthreads();
#pragma unroll
		for (int32_t ii = 0; ii < 4; ++ii)
#pragma unroll
			for (int32_t jj = 0; jj < 8; ++jj) st[(ty + 16 * ii) * DIST_OUTW + tx + 16 * jj] = (int32_t)acc[h * 4 + ii][jj];
		__syncthreads();
		for (int32_t e = t; e < DIST_TILE * DIST_TILE / 2; e += BLOCK) {
			const int32_t r = e >> 7, cc = e & 127, gi = i0 + h * 64 + r, gj = j0 + cc;
			if (gi < A && gj < A) {
				int32_t *p = S + (size_t)gi * An + (size_t)gj;
				if (add) atomicAdd(p, st[r * DIST_OUTW + cc]); else *p = st[r * DIST_OUTW + cc];
			}
		}
		if (ti == tj) continue;
		for (int32_t e = t; e < DIST_TILE * DIST_TILE / 2; e += BLOCK) {
			const int32_t cc = e >> 6, r = e & 63, gi = i0 + h * 64 + r, gj = j0 + cc;
			if (gi < A && gj < A) {
				int32_t *p = S + (size_t)gj * An + (size_t)gi;
				if (add) atomicAdd(p, st[r * DIST_OUTW + cc]); else *p = st[r * DIST_OUTW + cc];
			}
		}
	}
}
