// cloudsc2_parmap.hip -- per-column parameter maps (C2F_PARMAP): RKCONV, RCLCRIT, RLPTRC, RPECONS as (nblocks, nproma) fields.  The three
// launchers cloudsc2_{nl,tl,vjp}_launch_parmap and their kernels, which stay in the unit that launches them (cloudsc2_host.hpp): they are
// no rows of the table of cloudsc2_sweep_kernels.hpp, have no family number, no pacing, no launch-log entry and no nap.
//
// The kernels are the columns of their scalar parents -- cloudsc2_ad_launch_forward's nl_column, cloudsc2_tl_launch_par's tl_column,
// cloudsc2_vjp_launch_par's ad_reverse_column -- under the parents' launch bounds and variant words, with C2F_PARMAP added: a lane loads
// its four doubles from the value table before the level loop, derives its constants (lane_consts) and hands them to the level functions
// in place of the launch's.  Contract: column c of everything a launcher writes is the bits of its parent given a parameter block that
// holds column c's four values; the adjoint table is, per active column, that column's row of cloudsc2_vjp_launch_par's workspace.
#include "cloudsc2_host.hpp"

namespace cloudsc2 {

template <unsigned F>
__global__ void __launch_bounds__(kBlock, nl_waves_per_simd(F)) nl_parmap_kernel(NlParmapArgs args) {
  C2_KERNEL_BODY((nl_column<F | C2F_PARMAP>(global_column(), &kernarg<NlParmapArgs>()->a)));
}
template <unsigned F>
__global__ void __launch_bounds__(kBlock, tl_waves_per_simd(F)) tl_parmap_kernel(TlParmapArgs args) {
  C2_KERNEL_BODY((tl_column<F | C2F_PARMAP>(global_column(), &kernarg<TlParmapArgs>()->a)));
}
template <unsigned F>
__global__ void __launch_bounds__(kBlock, 1) vjp_parmap_kernel(AdParmapArgs args) {
  C2_KERNEL_BODY((ad_reverse_column<F | C2F_PARMAP>(global_column(), &kernarg<AdParmapArgs>()->a)));
}
// the variant words are the ensemble's: 16 kernels each per precision
C2_DEFINE_VARIANT(nl_parmap, NlParmapArgs, 64, nl_ens_variant_valid, kNone, kNone, false)
C2_DEFINE_VARIANT(tl_parmap, TlParmapArgs, 512, tl_par_variant_valid, kNone, kNone, false)
C2_DEFINE_VARIANT(vjp_parmap, AdParmapArgs, 512, vjp_par_variant_valid, kNone, kNone, false)

namespace {

// What the three launchers refuse first, in this order, all of it before the device is looked for.
int check_parmap(const cloudsc2_params* prm, int satur, int nproma, int nlev, int ngptot, const void* table, bool blocks_given) {
  if (!prm) return fail(CLOUDSC2_EINVAL, "params is NULL");
  if (!table) return fail(CLOUDSC2_EINVAL, "parameter maps: a table is NULL");
  if (int rc = check_satur(satur)) return rc;
  if (!prm->lphylin)
    return fail(CLOUDSC2_EINVAL, "parameter maps: CLOUDSC2TL / CLOUDSC2AD linearise the LPHYLIN form only (prm->lphylin = 0)");
  if (int rc = check_geom_args(prm, nproma, nlev, ngptot)) return rc;
  return blocks_given ? 0 : fail(CLOUDSC2_EINVAL, "NULL argument block");
}
int check_qsat(int satur, const cloudsc2_inputs* traj_in, const cloudsc2_inputs* other_in) {
  if (satur && (traj_in->qsat.ptr || other_in->qsat.ptr))
    return fail(CLOUDSC2_EINVAL, "satur = 1: SATUR is differentiated in the sweep, every qsat field must be NULL");
  return require_qsat(satur, traj_in);
}

}  // namespace
}  // namespace cloudsc2

using namespace cloudsc2;

extern "C" {

int cloudsc2_nl_launch_parmap(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot, const double* par_dev,
                              const cloudsc2_inputs* traj_in, const cloudsc2_outputs* traj_out, cloudsc2_real* scratch, void* stream) {
  int rc = check_parmap(prm, 0, nproma, nlev, ngptot, par_dev, traj_in && traj_out);
  if (rc) return rc;
  Sweep w;
  fill_geom(w.g, nproma, nlev, ngptot);
  if ((rc = w.trajectory(*traj_in, *traj_out, true))) return rc;
  const bool evap = prm->levapls2 || prm->ldrain1d;
  if (evap && !scratch) return fail(CLOUDSC2_EINVAL, "LEVAPLS2/LDRAIN1D: the cover-checkpoint plane `scratch` is required");
  if ((rc = require_device())) return rc;
  if ((rc = w.finish(*prm, ptsphy, traj_in->qsat.ptr, {(long long)nproma * nlev /* scratch */}))) return rc;
  NlParmapArgs args;
  args.a = w.nl();
  args.a.ckpt = scratch;
  args.par = par_dev; args.ptsphy = ptsphy;
  const unsigned f = w.f | (w.c.evap ? C2F_CKPT : 0u);  // the cover checkpoint exactly with the evaporation branch
  return launch_kernel(nl_parmap_variant(f), args, grid_for(w.g.ncols_pad, kBlock), (hipStream_t)stream);
}

int cloudsc2_tl_launch_parmap(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot, int satur, const double* par_dev,
                              const double* dpar_dev, const cloudsc2_inputs* traj_in, const cloudsc2_inputs* pert_in,
                              const cloudsc2_outputs* pert_out, void* stream) {
  int rc = check_parmap(prm, satur, nproma, nlev, ngptot, par_dev && dpar_dev ? par_dev : nullptr, traj_in && pert_in && pert_out);
  if (rc) return rc;
  if ((rc = check_qsat(satur, traj_in, pert_in))) return rc;
  Sweep w;
  fill_geom(w.g, nproma, nlev, ngptot);
  const cloudsc2_outputs none = {};
  if ((rc = w.trajectory(*traj_in, none, false))) return rc;
  TlParmapArgs args;
  TlArgs& a = args.a;
  a.sp = Strides{0, 0, 0, 0, 0};
  if ((rc = resolve_in(*pert_in, !satur, a.sp, a.din))) return rc;
  if ((rc = resolve_out(*pert_out, true, a.sp, a.dout))) return rc;
  if ((rc = require_device())) return rc;
  const Strides& sp = a.sp;
  if ((rc = w.finish(*prm, ptsphy, traj_in->qsat.ptr, {sp.full, sp.half, sp.cml, sp.clv, sp.loc}))) return rc;
  a.c = w.c; a.g = w.g; a.s = w.s; a.in = w.in; a.out = w.out; a.tab = w.tab;
  a.supsat_inc = RC(0.0); a.yy = nullptr;
  args.par = par_dev; args.dpar = dpar_dev; args.ptsphy = ptsphy;
  const unsigned f = w.f | (satur ? C2F_SATLIN : 0u) | C2F_PARLIN;
  return launch_kernel(tl_parmap_variant(f), args, grid_for(w.g.ncols_pad, kBlock), (hipStream_t)stream);
}

int cloudsc2_vjp_launch_parmap(const cloudsc2_params* prm, double ptsphy, int nproma, int nlev, int ngptot, int satur, const double* par_dev,
                               const cloudsc2_inputs* traj_in, const cloudsc2_outputs* traj_out, const cloudsc2_inputs* adj_in,
                               const cloudsc2_outputs* adj_out, const cloudsc2_real* scratch, double* par_adj_dev, void* stream) {
  int rc = check_parmap(prm, satur, nproma, nlev, ngptot, par_dev && par_adj_dev ? par_dev : nullptr, traj_in && traj_out && adj_in && adj_out);
  if (rc) return rc;
  if ((rc = check_qsat(satur, traj_in, adj_in))) return rc;
  Sweep w;
  fill_geom(w.g, nproma, nlev, ngptot);
  // the reverse sweep reads PFPLSL5 / PFPLSN5 and nothing else of the trajectory outputs
  if ((rc = w.trajectory(*traj_in, *traj_out, false))) return rc;
  if (!w.out.fplsl || !w.out.fplsn) return fail(CLOUDSC2_EINVAL, "reverse sweep: traj_out->fplsl and ->fplsn (PFPLSL5, PFPLSN5) are required");
  AdParmapArgs args;
  memset(&args, 0, sizeof(args));
  AdArgs& a = args.a;
  InPtrs aip_c;
  if ((rc = resolve_in(*adj_in, !satur, a.sa, aip_c))) return rc;
  if ((rc = resolve_out(*adj_out, true, a.sa, a.aout))) return rc;
  a.ain = writable(*adj_in);
  const bool evap = prm->levapls2 || prm->ldrain1d;
  if (evap && !scratch) return fail(CLOUDSC2_EINVAL, "LEVAPLS2/LDRAIN1D: the cover-checkpoint plane `scratch` is required");
  if ((rc = require_device())) return rc;
  const Strides& sa = a.sa;
  if ((rc = w.finish(*prm, ptsphy, traj_in->qsat.ptr, {sa.full, sa.half, sa.cml, sa.clv, sa.loc, (long long)nproma * nlev /* scratch */})))
    return rc;
  a.nl = w.nl();
  a.nl.ckpt = const_cast<cloudsc2_real*>(scratch);
  args.par = par_dev; args.apar = par_adj_dev; args.ptsphy = ptsphy;
  const unsigned f = w.f | C2F_ASSIGN | C2F_VJP | (satur ? C2F_SATLIN : 0u) | C2F_PARLIN;
  return launch_kernel(vjp_parmap_variant(f), args, grid_for(w.g.ncols_pad, kBlock), (hipStream_t)stream);
}

}  // extern "C"
