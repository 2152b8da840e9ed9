// ------------------------------------------------------------------------------------------------
// The permutation front of the pan commands: k_trait_perm (and with it k_perma_*), k_qtrait_perm and
// k_mantel_order make the rows of one batch of permutations here and differ only in what a row holds.
//   swaps  perm_swaps: the swap sequence curves pins (pgx::fisher_yates_order: Fisher-Yates from the last column down,
//          j = next() % (i + 1), splitmix64 from mix((seed << 32) | p)); the 64-bit % is the compiler's: the same j as the host's for
//          every x.
//   rows   perm_wave_rows: ONE wave, one lane per permutation, each lane over a private row of `elems` elements.  The 64 rows of a wave
//          are lane-interleaved, element k of lane l at k * 64 + l: a wave's access to "its" element i is one contiguous line, and the
//          accesses to the elements j spread over the LDS banks by lane.  The rows live in LDS while 64 of them fit 32 KiB
//          (elems <= LDS_ELEMS) and in a global scratch buffer work[workgroup][elems][64] of the same layout beyond.
// ------------------------------------------------------------------------------------------------
template <class Swap> __device__ __forceinline__ void perm_swaps(int32_t N, uint32_t seed, uint32_t p, Swap swap)
{
	uint64_t x = mix64((uint64_t)seed << 32 | (uint64_t)p);
	for (int32_t i = N - 1; i >= 1; --i) {
		x += 0x9E3779B97F4A7C15ull;
		swap(i, (int32_t)(mix64(x) % (uint64_t)(i + 1)));
	}
}

// the two steps more than one kernel uses: swap the elements i and j of a lane's row, and write a finished row row-major
struct PermSwapValues {
	template <class T> __device__ __forceinline__ void operator()(T *row, int32_t i, int32_t j) const
	{
		const T vi = row[i * WAVE], vj = row[j * WAVE];
		row[i * WAVE] = vj;
		row[j * WAVE] = vi;
	}
};
template <class T> __device__ __forceinline__ void perm_row_major(const T *fin, T *out, int32_t elems, int32_t l)
{
	for (int32_t k = l; k < elems; k += WAVE) out[k] = fin[k * WAVE];
}

// grid: ceil(nb / 64) workgroups of ONE wave; permutation p0 + q of the batch, q < nb, is row q.  fill(k): element k of every row
// before the swaps; swap(row, i, j): one swap of perm_swaps over the lane's row, element k at row[k * WAVE], for the columns
// n_swap - 1 .. 1 (n_swap = 0: no swaps); row_out(fin, q, l): lane l's share of writing out row q of the batch, element k at
// fin[k * WAVE].  Lanes past nb run a permutation nobody reads and write nothing.
template <class T, int32_t LDS_ELEMS, bool USE_LDS, class Fill, class Swap, class RowOut>
__device__ __forceinline__ void perm_wave_rows(int32_t elems, int32_t n_swap, uint32_t seed, uint32_t p0, int32_t nb, T *work, Fill fill, Swap swap, RowOut row_out)
{
	__shared__ T sh[USE_LDS ? LDS_ELEMS * WAVE : 1];
	const int32_t l = (int32_t)threadIdx.x;
	const int64_t q0 = (int64_t)blockIdx.x * WAVE;
	T *mine = USE_LDS ? sh : work + (size_t)blockIdx.x * (size_t)elems * WAVE;
	for (int32_t k = 0; k < elems; ++k) mine[k * WAVE + l] = fill(k);
	perm_swaps(n_swap, seed, p0 + (uint32_t)(q0 + l), [&](int32_t i, int32_t j) { swap(mine + l, i, j); });
	if (USE_LDS) __syncthreads(); // (one wave: orders the lanes' LDS stores before the reads across lanes below)
	else __threadfence_block();
	const int32_t n_row = (int32_t)min((int64_t)WAVE, (int64_t)nb - q0);
	for (int32_t q = 0; q < n_row; ++q) row_out(mine + q, q0 + q, l);
}

// The same rows written out element-major: out[k * stride + q], q = 64 blockIdx.x + l -- which is the wave's own layout, so the
// write-out is a copy of the block, a lane moving its own elements (no exchange across lanes, no barrier), 128 contiguous bytes of uint16
// per element and wave.  out has ceil(nb / 64) * 64 columns: the lanes past nb write the permutation nobody reads.
template <class T, int32_t LDS_ELEMS, bool USE_LDS, class Fill, class Swap>
__device__ __forceinline__ void perm_wave_block(int32_t elems, int32_t n_swap, uint32_t seed, uint32_t p0, T *work, Fill fill, Swap swap, T *out, size_t stride)
{
	__shared__ T sh[USE_LDS ? LDS_ELEMS * WAVE : 1];
	const int32_t l = (int32_t)threadIdx.x;
	const int64_t q0 = (int64_t)blockIdx.x * WAVE;
	T *mine = USE_LDS ? sh : work + (size_t)blockIdx.x * (size_t)elems * WAVE;
	for (int32_t k = 0; k < elems; ++k) mine[k * WAVE + l] = fill(k);
	perm_swaps(n_swap, seed, p0 + (uint32_t)(q0 + l), [&](int32_t i, int32_t j) { swap(mine + l, i, j); });
	T *col = out + (size_t)(q0 + l);
	for (int32_t k = 0; k < elems; ++k) col[(size_t)k * stride] = mine[k * WAVE + l];
}
