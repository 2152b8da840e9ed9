// ------------------------------------------------------------------------------------------------
// Principal coordinates (pga_pan_pcoa; DESIGN.md section 8 "Principal coordinates"): Lanczos with full reorthogonalisation for the
// largest eigenpairs of B = J A J, A = -1/2 d o d, d = q 2^-F.  B is never formed: for x orthogonal to 1, B x = A x - mean(A x) 1.
// The project's first floating-point kernels.  Every sum below has a fixed shape -- a lane's own terms in index order, the xor butterfly
// of the wave (both partners add the same two numbers, so every lane holds the same bits), the waves' partial sums in wave order -- and
// there is no floating-point atomic: the same launch returns the same bits however the workgroups are scheduled.
//   mult    k_pcoa_mult<B>: Y = A X for X[N][B], 1 <= B <= 8.  A workgroup takes PC_ROWS rows of q; a lane reads four consecutive
//           columns of each row as one 16-byte load (the rows are padded to a multiple of four columns, the padding is zero), turns them
//           into doubles, squares them and multiplies into B accumulators a row; the factor -2^(-2F - 1) is applied once, to the row's
//           sum (a power of two: the same bits as scaling every term).  q is read once per product; the mirror half is not exploited.
//   center  k_pcoa_center: one workgroup a column of Y subtracts the column's mean.
//   start   k_pcoa_start: a start vector from the counter (seed, restart, i), uniform in [-1/2, 1/2).
//   dots    k_pcoa_dots: c[i] = V[i] . w, one workgroup a vector, all earlier vectors in one launch.
//   update  k_pcoa_update: w -= sum over i of c[i] V[i], a lane an element, the vectors in index order.
//   norm    k_pcoa_norm: one workgroup.  beta = |w|; alpha and beta of the step are recorded; |B v| of the step, rebuilt from the
//           coefficients, raises the running estimate of |B|; beta <= 1e-12 times that estimate sets the "broke down" flag, otherwise w
//           becomes the next vector.  Every kernel of a step returns at once when the flag is set, so the steps a chunk still has queued
//           behind a breakdown are no-ops; the host reads alpha, beta and the flag once per chunk and decides there.
//   ritz    k_pcoa_ritz: X = V S for the selected columns.
// ------------------------------------------------------------------------------------------------
constexpr int32_t PC_ROWS = 4;       // rows of q a workgroup of k_pcoa_mult takes: X is read once for four rows
constexpr int32_t PC_MAX_B = 8;      // columns of X at the most
constexpr int32_t PC_MAX_VEC = 256;  // Lanczos vectors at the most
constexpr double PC_BREAK = 1e-12;   // breakdown: beta <= PC_BREAK times the running estimate of |B|

struct PcoaState { double norm_est; int32_t broke, n_done; }; // the running estimate of |B|; a step broke down; the steps that ran

__device__ __forceinline__ double pc_wave_sum(double v) // every lane gets the same bits
{
#pragma unroll
	for (int d = WAVE / 2; d >= 1; d >>= 1) v += __shfl_xor(v, d, WAVE);
	return v;
}

// part[BLOCK / WAVE]; every thread gets the sum: the waves' sums added in wave order
__device__ __forceinline__ double pc_block_sum(double v, double *part)
{
	v = pc_wave_sum(v);
	__syncthreads(); // (part may still be read from the call before)
	if ((threadIdx.x & (WAVE - 1)) == 0) part[threadIdx.x / WAVE] = v;
	__syncthreads();
	double s = part[0];
#pragma unroll
	for (int k = 1; k < BLOCK / WAVE; ++k) s += part[k];
	return s;
}

// grid: ceil(N / PC_ROWS).  q[N][ld], ld a multiple of 4 and the columns from N on zero; x[ld][B] with the rows from N on zero;
// y[N][B] = scale * sum over c of q[r][c]^2 x[c][.]
template <int B>
__global__ __launch_bounds__(BLOCK) void k_pcoa_mult(const int32_t *__restrict__ q, int32_t N, int32_t ld, double scale, const double *__restrict__ x,
                                                     double *__restrict__ y, const PcoaState *__restrict__ st)
{
	__shared__ double part[PC_ROWS * B][BLOCK / WAVE];
	if (st->broke) return;
	const int32_t t = (int32_t)threadIdx.x, r0 = (int32_t)blockIdx.x * PC_ROWS;
	const int32_t *row[PC_ROWS];
#pragma unroll
	for (int i = 0; i < PC_ROWS; ++i) row[i] = q + (size_t)min(r0 + i, N - 1) * (size_t)ld; // (a row past the end repeats the last one and is not stored)
	double acc[PC_ROWS][B];
#pragma unroll
	for (int i = 0; i < PC_ROWS; ++i)
#pragma unroll
		for (int k = 0; k < B; ++k) acc[i][k] = 0.0;
	for (int32_t c = 4 * t; c < ld; c += 4 * BLOCK) {
		int4 v[PC_ROWS];
#pragma unroll
		for (int i = 0; i < PC_ROWS; ++i) v[i] = *(const int4 *)(row[i] + c);
		double s[PC_ROWS][4];
#pragma unroll
		for (int i = 0; i < PC_ROWS; ++i) {
			const double d0 = (double)v[i].x, d1 = (double)v[i].y, d2 = (double)v[i].z, d3 = (double)v[i].w;
			s[i][0] = d0 * d0, s[i][1] = d1 * d1, s[i][2] = d2 * d2, s[i][3] = d3 * d3;
		}
#pragma unroll
		for (int j = 0; j < 4; ++j) {
			double xv[B];
#pragma unroll
			for (int k = 0; k < B; ++k) xv[k] = x[(size_t)(c + j) * B + k];
#pragma unroll
			for (int i = 0; i < PC_ROWS; ++i)
#pragma unroll
				for (int k = 0; k < B; ++k) acc[i][k] = fma(s[i][j], xv[k], acc[i][k]);
		}
	}
#pragma unroll
	for (int i = 0; i < PC_ROWS; ++i)
#pragma unroll
		for (int k = 0; k < B; ++k) {
			const double w = pc_wave_sum(acc[i][k]);
			if ((t & (WAVE - 1)) == 0) part[i * B + k][t / WAVE] = w;
		}
	__syncthreads();
	if (t < PC_ROWS * B && r0 + t / B < N) {
		double sum = part[t][0];
#pragma unroll
		for (int k = 1; k < BLOCK / WAVE; ++k) sum += part[t][k];
		y[(size_t)(r0 + t / B) * B + (t % B)] = scale * sum;
	}
}

// grid: b, one workgroup a column: y[N][b], y[.][k] -= its mean
__global__ __launch_bounds__(BLOCK) void k_pcoa_center(double *__restrict__ y, int32_t N, int32_t b, const PcoaState *__restrict__ st)
{
	__shared__ double part[BLOCK / WAVE];
	if (st->broke) return;
	const int32_t t = (int32_t)threadIdx.x, k = (int32_t)blockIdx.x;
	double s = 0.0;
	for (int32_t r = t; r < N; r += BLOCK) s += y[(size_t)r * b + k];
	const double mean = pc_block_sum(s, part) / (double)N;
	for (int32_t r = t; r < N; r += BLOCK) y[(size_t)r * b + k] -= mean;
}

// grid: ceil(N / 256).  w[i] = the uniform number of the counter (seed, restart, i), in [-1/2, 1/2)
__global__ __launch_bounds__(BLOCK) void k_pcoa_start(double *__restrict__ w, int32_t N, uint32_t seed, uint32_t restart)
{
	const int32_t i = (int32_t)(blockIdx.x * BLOCK + threadIdx.x);
	if (i >= N) return;
	const uint64_t x = mix64((uint64_t)seed << 32 | (uint64_t)restart) + ((uint64_t)i + 1) * 0x9E3779B97F4A7C15ull;
	w[i] = (double)(mix64(x) >> 11) * 0x1p-53 - 0.5;
}

// grid: m, one workgroup a vector: c[i] = V[i] . w with V[m][ld]
__global__ __launch_bounds__(BLOCK) void k_pcoa_dots(const double *__restrict__ V, int32_t ld, int32_t N, const double *__restrict__ w, double *__restrict__ c,
                                                     const PcoaState *__restrict__ st)
{
	__shared__ double part[BLOCK / WAVE];
	if (st->broke) return;
	const int32_t t = (int32_t)threadIdx.x;
	const double *v = V + (size_t)blockIdx.x * (size_t)ld;
	double s = 0.0;
	for (int32_t r = t; r < N; r += BLOCK) s = fma(v[r], w[r], s);
	s = pc_block_sum(s, part);
	if (t == 0) c[blockIdx.x] = s;
}

// grid: ceil(N / 256).  w[r] -= sum over i < m of c[i] V[i][r], in the order of i
__global__ __launch_bounds__(BLOCK) void k_pcoa_update(const double *__restrict__ V, int32_t ld, int32_t N, int32_t m, const double *__restrict__ c, double *__restrict__ w,
                                                       const PcoaState *__restrict__ st)
{
	if (st->broke) return;
	const int32_t r = (int32_t)(blockIdx.x * BLOCK + threadIdx.x);
	if (r >= N) return;
	double s = 0.0;
	for (int32_t i = 0; i < m; ++i) s = fma(c[i], V[(size_t)i * (size_t)ld + r], s);
	w[r] -= s;
}

// grid: 1.  j >= 0: the end of step j over its m = j + 1 coefficients of the two passes c1, c2: alpha[j] = c1[j] + c2[j], beta[j] = |w|,
// the breakdown test, and w /= beta when it passes.  j < 0: a start vector is normalised (a zero vector sets the flag to 2).
__global__ __launch_bounds__(BLOCK) void k_pcoa_norm(double *__restrict__ w, int32_t N, int32_t j, const double *__restrict__ c1, const double *__restrict__ c2,
                                                     double host_est, double *__restrict__ alpha, double *__restrict__ beta, PcoaState *__restrict__ st)
{
	__shared__ double part[BLOCK / WAVE];
	if (st->broke) return;
	const int32_t t = (int32_t)threadIdx.x;
	const double est0 = st->norm_est;
	double s = 0.0;
	for (int32_t r = t; r < N; r += BLOCK) s = fma(w[r], w[r], s);
	const double b = sqrt(pc_block_sum(s, part)); // (the barriers inside stand between the read of st above and the writes below)
	if (j < 0) {
		if (b > 0.0) { const double inv = 1.0 / b; for (int32_t r = t; r < N; r += BLOCK) w[r] *= inv; }
		else if (t == 0) st->broke = 2;
		return;
	}
	double raw = b * b; // |B v_j|^2 = the squares of its coefficients over the vectors so far, and of what is left
	for (int32_t i = 0; i <= j; ++i) { const double ci = c1[i] + c2[i]; raw = fma(ci, ci, raw); }
	const double est = fmax(fmax(est0, host_est), sqrt(raw));
	const bool broke = b <= PC_BREAK * est;
	if (t == 0) {
		alpha[j] = c1[j] + c2[j], beta[j] = b;
		st->norm_est = est, st->n_done += 1;
		if (broke) st->broke = 1;
	}
	if (!broke) { const double inv = 1.0 / b; for (int32_t r = t; r < N; r += BLOCK) w[r] *= inv; }
}

// grid: (ceil(N / 256), ka).  x[N][ka]: x[r][a] = sum over i < m of S[a][i] V[i][r], in the order of i
__global__ __launch_bounds__(BLOCK) void k_pcoa_ritz(const double *__restrict__ V, int32_t ld, int32_t N, int32_t m, const double *__restrict__ S, int32_t ka, double *__restrict__ x)
{
	const int32_t r = (int32_t)(blockIdx.x * BLOCK + threadIdx.x), a = (int32_t)blockIdx.y;
	if (r >= N) return;
	const double *s = S + (size_t)a * (size_t)m;
	double sum = 0.0;
	for (int32_t i = 0; i < m; ++i) sum = fma(s[i], V[(size_t)i * (size_t)ld + r], sum);
	x[(size_t)r * ka + a] = sum;
}
