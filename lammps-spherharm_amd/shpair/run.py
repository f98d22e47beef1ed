"""Device-resident timestep loop over the C ABI (include/shpair.h + include/shstep.h).

The host-side mirror of what LAMMPS' Verlet::run does around PairSH::compute for ONE rank whose atoms
live in HBM: initial_integrate -> neighbour decide (borders + build when an atom moved skin/2) -> clear ->
the force pass both drivers share (step_pass.force_pass: forward ghosts ... body forces) -> final_integrate.  Every
array stays on the GPU; torch only owns the memory.  LAMMPS itself is out of scope;
this driver exists so that tests and bench.py can time and check whole steps.
"""
import numpy as np
import torch

from .step_pass import StepView, apply_contact_options, force_pass, rank_arrays


class DeviceRun:
    def __init__(self, sp, x, quat, shtype, lo, hi, periodic, skin, type_=None, dt=1e-3, gravity=(0.0, 0.0, 0.0),
                 gamma_t=0.0, gamma_r=0.0, mask=None, groupbit=1, ghost_factor=None, device="cuda:0", check=True, ledger=False,
                 shell_ledger=None, **contact):
        """ledger: switches the context's energy ledger on (docs/SPEC.md §2.13); step() and run_native() then fold once
        per step and ledger() reads the tally back.
        shell_ledger: the switch of the ledger's cylinder entries (§2.20), set ahead of the contact options; with
        ledger=True, shell_ledger=True a drum with damping, friction or springs keeps its dissipation and drive work, and
        shell_ledger() reads them back.  None leaves the context's switch as it is.
        contact: walls, pair_damping, wall_damping, pair_friction, wall_friction, wall_velocity, pair_spring, wall_spring,
        pair_rolling, pair_twisting, wall_rolling, wall_twisting, cylinders, cylinder_damping, cylinder_friction,
        cylinder_rotation, cylinder_spring, cylinder_rolling, cylinder_twisting, cones, cone_damping, cone_friction,
        cone_rotation, conic_spring, conic_rolling, conic_twisting, as step_pass.apply_contact_options takes them (None leaves the context's as they are)."""
        self.sp, self.dt, self.groupbit, self.check = sp, float(dt), int(groupbit), check
        self.g = tuple(float(c) for c in gravity)
        self.gamma_t, self.gamma_r = float(gamma_t), float(gamma_r)
        n = x.shape[0]
        self.n = n
        if ghost_factor is None:
            # ghosts live in a shell of one ghost cutoff around the periodic faces
            ext = np.asarray(hi, float) - np.asarray(lo, float)
            cm = 2.0 * max(sp.rmax(s) for s in range(sp.nshapes)) + skin
            shell = np.prod(ext + 2.0 * cm * np.asarray(periodic, float)) / np.prod(ext)
            ghost_factor = 1.3 * shell + 0.05
        self.nmax = int(n * ghost_factor) + 64
        rank_arrays(self, device, n, self.nmax, n, x, quat, shtype, type_=type_, mask=mask)
        self.nghost = 0
        self.npairs = 0
        self.builds = 0
        self.steps = 0
        sp.set_box(lo, hi, periodic, skin)
        apply_contact_options(sp, shell_ledger=shell_ledger, **contact)
        if ledger:
            sp.set_energy_ledger(True)
        # (w, omega) of owned and ghost rows, docs/SPEC.md §2.10: only while the context holds a coefficient, whoever set it
        self.twist = torch.zeros(self.nmax, 6, dtype=torch.float64, device=self.dev) if sp.has_dissipation else None
        # the pointers of a StepView, x ... twist: the tensors stay where they are
        tensors = (self.x, self.q, self.v, self.L, self.ty, self.sh, self.mask, self.f, self.tq, self.twist)
        self._ptrs = tuple(None if t is None else t.data_ptr() for t in tensors)
        self.rebuild()
        self.force()

    # -- pieces ---------------------------------------------------------------------------------
    def rebuild(self):
        sp = self.sp
        self.nghost = sp.borders_device(self.n, self.nmax, self.x.data_ptr(), self.q.data_ptr(), self.ty.data_ptr(),
                                        self.sh.data_ptr())
        self.npairs = sp.neighbor_build_device(self.n, self.nghost, self.x.data_ptr(), self.sh.data_ptr())
        self.builds += 1

    def force(self, eflag=False, advance=False):
        """advance: the force pass of a step — the planes of translating walls move by dt ahead of the wall pass."""
        sp = self.sp
        self.f.zero_()
        self.tq.zero_()
        if eflag:
            self.ev.zero_()
        v = StepView(self.n, self.nghost, *self._ptrs, self.groupbit, self.dt, self.g, self.gamma_t, self.gamma_r, None)
        # the ghosts are the context's own periodic images: the twist kernel fills their rows from their owners'
        force_pass(sp, v, lambda twist: sp.forward_device(v.x, v.quat), lambda: sp.reverse_device(v.f, v.torque), self.nghost,
                   eflag=eflag, ev=self.ev.data_ptr(), advance=advance)

    def _nve(self, phase):
        self.sp.nve_device(phase, self.n, self.dt, self.x.data_ptr(), self.v.data_ptr(), self.q.data_ptr(),
                           self.L.data_ptr(), self.f.data_ptr(), self.tq.data_ptr(), self.sh.data_ptr(),
                           self.mask.data_ptr(), groupbit=self.groupbit)

    # -- Verlet::run ----------------------------------------------------------------------------
    def step(self, eflag=False):
        self._nve(0)
        if self.check and self.sp.neighbor_check_device(self.n, self.x.data_ptr()):
            self.rebuild()
        self.force(eflag, advance=True)
        if self.sp.ledger_on:      # as step_after_reverse: dt times the powers this step's passes left, once per step
            self.sp.ledger_fold_device(self.dt)
        self._nve(1)
        self.steps += 1

    def run(self, nsteps, eflag_last=False):
        for k in range(nsteps):
            self.step(eflag=eflag_last and k == nsteps - 1)

    def run_native(self, nsteps, use_graph=False, check_every=1):
        """The same loop inside the library (shstep_run_device): C++ host code, optionally replayed from
        captured hipGraphs — for small, launch-bound systems.  Runs on the context's own stream."""
        from .capi import StepArrays
        a = StepArrays()
        a.nlocal, a.nmax = self.n, self.nmax
        a.x, a.v, a.quat, a.angmom = self.x.data_ptr(), self.v.data_ptr(), self.q.data_ptr(), self.L.data_ptr()
        a.f, a.torque = self.f.data_ptr(), self.tq.data_ptr()
        a.type, a.shtype, a.mask = self.ty.data_ptr(), self.sh.data_ptr(), self.mask.data_ptr()
        a.groupbit, a.dt = self.groupbit, self.dt
        a.gravity = (self.g[0], self.g[1], self.g[2])
        a.gamma_t, a.gamma_r, a.check_every = self.gamma_t, self.gamma_r, int(check_every)
        torch.cuda.synchronize()          # everything enqueued on torch's stream is visible to the context's stream
        self.nghost, nreb = self.sp.run_device(a, nsteps, self.nghost, use_graph=use_graph, stream=self.sp.own_stream())
        self.builds += nreb
        self.steps += nsteps

    def contact_history(self):
        """xi [npairs][3] of the tangential springs (docs/SPEC.md §2.14), in the slot order of sp.copy_neighbors().  Blocks."""
        return self.sp.contact_history(self.n)

    def wall_history(self):
        """xi [n][nw][3] of the walls' tangential springs (docs/SPEC.md §2.15), 0 where nothing is live.  Blocks."""
        return self.sp.wall_history(self.n)

    def cylinder_history(self):
        """(xi_a, xi_theta) [n][nc][2] of the cylinders' tangential springs (docs/SPEC.md §2.19), 0 where nothing is live.
        Blocks."""
        return self.sp.cyl_history(self.n)

    def cone_history(self):
        """(xi_g, xi_theta, phi_c) [n][nk][3] of the cones' tangential springs (docs/SPEC.md §2.23), 0 where nothing is live:
        with get_cones() and the arrays what a restart needs (ShPair.set_conic_history puts it back).  Blocks."""
        return self.sp.conic_history(self.n)

    def ledger(self):
        """The energy ledger as a dict: the five time integrals by name, 'dissipated' (the first four), 'work', and
        'per_wall' [nw][3] = damping, friction, work.  Blocks."""
        tot, per = self.sp.energy_ledger()
        out = dict(zip(self.sp.LEDGER_TERMS, (float(t) for t in tot)))
        out.update(dissipated=float(tot[0] + tot[1] + tot[2] + tot[3]), work=float(tot[4]), per_wall=per)
        return out

    def shell_ledger(self):
        """The cylinder entries of the energy ledger (docs/SPEC.md §2.20) as a dict: 'damping', 'friction' (the energy the
        shells dissipated), 'work' (what the drives delivered) and 'per_cylinder' [nc][3] in the same order.  Blocks."""
        tot, per = self.sp.shell_ledger()
        out = dict(zip(self.sp.SHELL_TERMS, (float(t) for t in tot)))
        out.update(per_cylinder=per)
        return out

    def energies(self):
        """(contact energy of the last eflag force call, translational KE, rotational KE, gravitational PE)."""
        self.en.zero_()
        self.sp.energies_device(self.n, self.g, self.x.data_ptr(), self.v.data_ptr(), self.q.data_ptr(), self.L.data_ptr(),
                                self.sh.data_ptr(), self.mask.data_ptr(), self.en.data_ptr(), groupbit=self.groupbit)
        torch.cuda.synchronize()
        e = self.en.cpu().numpy()
        return float(self.ev[0].item()), float(e[0]), float(e[1]), float(e[2])
