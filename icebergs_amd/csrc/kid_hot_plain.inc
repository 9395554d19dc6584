// kid_hot_plain.inc -- launcher of the plain hot build of the fused RK4 step, berg_kernel<true, true, evolve|thermo|spread, true, K>
// with K = 1 (the bergs' environment is not stored) or K = 3 (it is); K = -1 / -3: their re-binning instances.  These two instantiations are compiled on their own
// (kid_hot_plain.hip) with LLVM's max-ILP machine scheduler: 158 registers instead of 160 and 2.7 % less time per launch at 1e7
// bergs (0.766 -> 0.752 ms); the same scheduler costs the footloose-profile build its third-wave register budget (155 -> 191)
// and slows the general build, so it is not a flag of the whole library.  A one-file build of kid_hip.hip (experiments) includes
// this file itself.  Flags / Redo / BergPtrs live in an anonymous namespace: they cross the boundary as untyped pointers.
namespace kid {
int launch_hot_plain(int K, unsigned nblocks, void *stream, const DevGrid *gtab, const kid_params *pp, const void *bp, long long n, double *acc,
                     size_t ncell, const void *flags, const void *redo) {
  constexpr unsigned PH = PH_EVOLVE | PH_THERMO | PH_SPREAD;
  const Flags &fl = *static_cast<const Flags *>(flags);
  const Redo &rd = *static_cast<const Redo *>(redo);
  if (K == 1)
    hipLaunchKernelGGL((berg_kernel<true, true, PH, true, 1>), dim3(nblocks), dim3(KID_HOT_WG), 0, (hipStream_t)stream, gtab, pp, static_cast<const BergPtrs *>(bp), n, acc, ncell, fl, rd);
  else if (K == 3)
    hipLaunchKernelGGL((berg_kernel<true, true, PH, true, 3>), dim3(nblocks), dim3(KID_HOT_WG), 0, (hipStream_t)stream, gtab, pp, static_cast<const BergPtrs *>(bp), n, acc, ncell, fl, rd);
  // the re-binning instances: the launch that follows a re-binning (redo.rb, redo.perm; kid_berg_kernel.hpp)
  else if (K == -1)
    hipLaunchKernelGGL((berg_kernel<true, true, PH, true, 1, false, true>), dim3(nblocks), dim3(KID_HOT_WG), 0, (hipStream_t)stream, gtab, pp, static_cast<const BergPtrs *>(bp), n, acc, ncell, fl, rd);
  else if (K == -3)
    hipLaunchKernelGGL((berg_kernel<true, true, PH, true, 3, false, true>), dim3(nblocks), dim3(KID_HOT_WG), 0, (hipStream_t)stream, gtab, pp, static_cast<const BergPtrs *>(bp), n, acc, ncell, fl, rd);
  else return -1;
  return 0;
}
}  // namespace kid
