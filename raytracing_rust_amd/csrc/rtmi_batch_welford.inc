// rtmi_batch_welford.inc — the sample loop of the batch modes' resolve kernels (rtmi_radiance.hip, rtmi_gather.hip,
// rtmi_sparse.hip), one lane per entry: the f64 sum of the entry's samples in sample order (the additions of
// rtmi_resolve_kernel) and Welford's recurrence in the operation order of rtmi_adaptive_resolve_kernel, the render's.
// A textual body, as rtmi_kernel_perlane.inc: a function, even force-inlined, moved the registers of the resolve kernels.
// The includer provides
//     const Rad3 *src             the entry's samples
//     const uint32_t ns           how many
//     double sum[3], m[3], M2[3]  zeroed; on exit the sum, the running mean and the sum of squared deviations per channel
for (uint32_t s = 0; s < ns; s++) {
    const Rad3 v = src[s];
    const double k = (double)(s + 1u);
    const double x[3] = {(double)v.r, (double)v.g, (double)v.b};
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
        sum[ch] += x[ch];
        const double dl = x[ch] - m[ch];
        m[ch] = m[ch] + dl / k;
        M2[ch] = M2[ch] + dl * (x[ch] - m[ch]);
    }
}
