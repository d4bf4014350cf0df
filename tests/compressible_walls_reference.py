"""CPU restatement of the compressible split-explicit model on walls in y — topology (Periodic, Bounded, Bounded), impenetrable south and
north walls, the reference's validation/cartesian_baroclinic_wave set-up.

TEST INFRASTRUCTURE ONLY.  oracle/oracle_compressible.py: CompressibleOracleModel stops after the walled acoustic loop (the fills with the
model's boundary conditions and compute_velocities! that close acoustic_rk3_substep_loop! are left to the caller there, as in the
library's bz_acoustic_substep_loop).  The subclass below restates the rest with the oracle's own C kernels, whose stencils are already
topology-aware (buffer_at(..., G->ty == BOUNDED)):

  fill_halo_regions! with the model's default conditions on a Bounded y: a field that is a centre in y takes the no-flux copy in its
  first halo rows; the y-face fields rho v, v and <v> get zeros on their wall faces 0 and Ny (face Ny lives in the first upper halo row);
  the tail of acoustic_rk3_substep_loop! (acoustic_substepping.jl:1560-1587): fills of rho_d, rho theta, rho u, rho v, rho w,
  compute_velocities!, fills of u, v, w.

On a (Periodic, Periodic, Bounded) grid every override reduces to the parent's code (the og_fill_halo_y_* calls return at once)."""
import ctypes as C

from oracle.oracle import BOUNDED, _p
from oracle.oracle_compressible import CompressibleOracleModel


class WalledCompressibleOracleModel(CompressibleOracleModel):
    def _is_yface(self, f):
        return any(f is getattr(self, n, None) for n in ("rv", "v", "av"))

    def _halo_y(self, f):
        n = C.c_int(f.shape[0])
        fill = self.lib.og_fill_halo_y_wall if self._is_yface(f) else self.lib.og_fill_halo_y_noflux
        fill(C.byref(self.cg), _p(f), n)

    def _halo_center(self, f):
        self.lib.og_fill_halo_periodic_xy(C.byref(self.cg), _p(f), C.c_int(f.shape[0]))
        self._halo_y(f)
        self.lib.og_fill_halo_z_noflux(C.byref(self.cg), _p(f))

    def _halo_w(self, f):
        self.lib.og_fill_halo_periodic_xy(C.byref(self.cg), _p(f), C.c_int(f.shape[0]))
        self.lib.og_fill_halo_y_noflux(C.byref(self.cg), _p(f), C.c_int(f.shape[0]))
        self.lib.og_fill_halo_z_wall(C.byref(self.cg), _p(f))

    def acoustic_substep_loop(self, dt, beta):
        super().acoustic_substep_loop(dt, beta)
        if self.grid.topo[1] != BOUNDED:
            return
        for f in (self.rho_d, self.rtheta, self.ru, self.rv):
            self._halo_center(f)
        self._halo_w(self.rw)
        self.lib.og_compute_velocities_3d(C.byref(self.cg), _p(self.u), _p(self.v), _p(self.w), _p(self.ru), _p(self.rv),
                                          _p(self.rw), _p(self.rho_d))
        self._halo_center(self.u)
        self._halo_center(self.v)
        self._halo_w(self.w)


def column_mass(om, name="rho_d"):
    """sum of field * dz over the interior (dx, dy uniform)"""
    import numpy as np
    g = om.grid
    return float((g.interior(getattr(om, name)) * np.asarray(g.dzc[g.Hz:g.Hz + g.Nz])[:, None, None]).sum())
