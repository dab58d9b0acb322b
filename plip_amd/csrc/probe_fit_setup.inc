// probe_fit_setup.inc -- the opening of a fit kernel (probe.hip probe_loss_grad_kernel<CT>, probe_softmax.hip
// softmax_loss_grad_kernel<CT, FUSED>), included as the first thing in the kernel body; probe_fit_walk.inc is the rest.  Text, not a
// function, like attention_flash_step.inc: these kernels sit at 256 VGPRs plus AGPRs, and only the text form keeps their instructions
// (profiles/embedding_tile_isa_diff.txt).  The including kernel provides CT, X, N, D, WB, and K = the number of problems (rows of WB);
// grid.y = the group of 16 problems this workgroup fits.
  using T = ProbeTile<CT>;
  constexpr int Dp = T::Dp;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* xs = lds;                                   // [32][Dp], swizzled
  float* zp = xs + kRows * Dp;                       // [4][32][16] partial scores; at the end: the loss / g_b reduction
  float* rs = zp + 4 * kRows * kGroup;               // [32][16] residuals

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int kbase = blockIdx.y * kGroup, KP = gridDim.y * kGroup;
  const long ntiles = ((long)N + kRows - 1) / kRows;

  // the W slice and the G accumulators stay in registers for the whole kernel
  float wf[T::KS];
  T::load_w(wf, WB, K, D, kbase, wave, lane);
  f32x4 g[CT];
#pragma unroll
  for (int j = 0; j < CT; ++j) g[j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // residual stage: this thread's problem and its two rows (rr, rr + 16) of a tile
  const int rc = tid & 15, rr = tid >> 4, cls = kbase + rc;
  const bool live = cls < K;
