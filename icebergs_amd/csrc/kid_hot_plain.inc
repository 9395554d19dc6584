// kid_hot_plain.inc -- launcher of the plain hot build of the fused RK4 step, berg_kernel<true, true, evolve|thermo|spread, true, K>
// with K = 1 (the bergs' environment is not stored) or K = 3 (store_env: it is); rebin: their re-binning instances.  These two instantiations are compiled on their own
// (kid_hot_plain.hip) with LLVM's max-ILP machine scheduler: 158 registers instead of 160 and 2.7 % less time per launch at 1e7
// bergs (0.766 -> 0.752 ms); the same scheduler costs the footloose-profile build its third-wave register budget (155 -> 191)
// and slows the general build, so it is not a flag of the whole library.  A one-file build of kid_hip.hip (experiments) includes
// this file itself.  Flags / Redo / BergPtrs live in an anonymous namespace: they cross the boundary as untyped pointers.
namespace kid {
void launch_hot_plain(bool store_env, bool rebin, unsigned nblocks, void *stream, const DevGrid *gtab, const kid_params *pp, const void *bp, long long n, double *acc,
                      size_t ncell, const void *flags, const void *redo) {
  constexpr unsigned PH = PH_EVOLVE | PH_THERMO | PH_SPREAD;
  const Flags &fl = *static_cast<const Flags *>(flags);
  const Redo &rd = *static_cast<const Redo *>(redo);
  const dim3 grid(nblocks), block(KID_HOT_WG);
  const hipStream_t s = (hipStream_t)stream;
  const BergPtrs *b = static_cast<const BergPtrs *>(bp);
  // rebin: the launch that follows a re-binning (redo.rb, redo.perm; kid_berg_kernel.hpp)
  if (!store_env && !rebin) hipLaunchKernelGGL((berg_kernel<true, true, PH, true, 1>), grid, block, 0, s, gtab, pp, b, n, acc, ncell, fl, rd);
  else if (store_env && !rebin) hipLaunchKernelGGL((berg_kernel<true, true, PH, true, 3>), grid, block, 0, s, gtab, pp, b, n, acc, ncell, fl, rd);
  else if (!store_env) hipLaunchKernelGGL((berg_kernel<true, true, PH, true, 1, false, true>), grid, block, 0, s, gtab, pp, b, n, acc, ncell, fl, rd);
  else hipLaunchKernelGGL((berg_kernel<true, true, PH, true, 3, false, true>), grid, block, 0, s, gtab, pp, b, n, acc, ncell, fl, rd);
}
}  // namespace kid
