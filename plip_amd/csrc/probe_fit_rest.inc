// probe_fit_rest.inc -- the rest of a fit kernel's walk, behind the kernel's residual stage (probe_fit_walk.inc): the residuals to LDS,
// phase 2 (G += R^T X_tile), the next tile; after the last one the workgroup's slot pg of part_g [gridDim.x][KP][D + 1].  `red` ([2][256]
// doubles over zp) is left for the kernel's own reduction of its loss terms and of the g_b terms into the slot's intercept column.
      rs[r * kGroup + rc] = res;
    }
    __syncthreads();
    // phase 2: G[problem][d] += sum_row R[row][problem] X[row][d]
    {
      const int m = lane & 15, k = lane >> 4;
#pragma unroll
      for (int q = 0; q < kRows / 4; ++q) {
        const int row = 4 * q + k;
        const float a = rs[row * kGroup + m];
        const float* xr = xs + row * Dp;
        const int sw = probe_swz(row);
#pragma unroll
        for (int j = 0; j < CT; ++j) g[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, xr[((wave * CT + j) * 16 + m) ^ sw], g[j], 0, 0, 0);
      }
    }
    __syncthreads();
    t = next;
  }

  // this workgroup's slot
  float* pg = part_g + ((size_t)blockIdx.x * KP + kbase) * (D + 1);
  {
    const int m = lane & 15, k = lane >> 4;
#pragma unroll
    for (int j = 0; j < CT; ++j) {
      const int d = (wave * CT + j) * 16 + m;
      if (d < D) {
#pragma unroll
        for (int i = 0; i < 4; ++i) pg[(size_t)(4 * k + i) * (D + 1) + d] = g[j][i];     // C/D: row (problem) = 4 (lane >> 4) + i
      }
    }
  }
  double* red = reinterpret_cast<double*>(zp);        // [2][16 row slots][16 problems] doubles = 4 KiB of zp's 8 KiB
