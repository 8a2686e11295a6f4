#!/usr/bin/env python3
"""Golden vectors for the RFCavity: tests/golden/dkd_rfcavity.npz.

Run in the build container only (imports the reference read-only through generate_golden.py):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/generate_golden_dkd_rfcavity.py

The reference has no storage-ring cavity. Its Bmad-X module has the building blocks, and this script composes Bmad's `rfcavity`
(bmad_standard) from them in float64 (DATA only in the file: inputs, parameters, outputs):

    cheetah_to_bmad_coords                          (tau, delta) -> (z, pz), once
    track_a_drift(L / 2)
    t = particle_rf_time(z, pz)                     = -z / (beta c), the particle's time offset tau / c
    dE = |n_q| V sin(2 pi (phase - f t))            the sine taken directly: no reduction, no addition theorem (|f t| < 4 here)
    E_new = pc / beta + dE,  pc_new = sqrt(E_new^2 - m^2),  pz = (pc_new - p0c) / p0c,  z = z beta_new / beta
    track_a_drift(L / 2)
    bmad_to_cheetah_coords                          (z, pz) -> (tau, delta), once; the reference energy is NOT changed

Cases: phase 0, 0.5 and 0.13 (units of 2 pi) with L = 0 and 0.3 m on electrons at 100 MeV; a proton beam at 2 GeV with phase 0.13
(L = 0, 0.3) and 0.5 (L = 0.3). f = 480 MHz, V = 1 MV. Two beams of 257 particles per species: "short" (sigma_tau = 1 cm, |f t| <
0.1) and "long" (sigma_tau = 1 m: |f t| > 1 for a third of the rows, which exercises the phase reduction). The last row of the
"long" beam has a kinetic energy of 100 keV and stands a quarter period behind the zero crossing of phase 0.13: in seven of the
nine cases (the half drift in front of the kick moves so slow a particle by a fifth of a period) it is decelerated by more than
that, its total energy behind the kick is below the rest mass, and the row is NaN in x, y, tau, delta (px, py are not touched).
"""

import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from generate_golden import cheetah, np, npy, save, species_meta, torch  # noqa: E402

from cheetah.utils import bmadx  # noqa: E402

F64 = {"dtype": torch.float64}
N = 257
FREQUENCY = 480e6
VOLTAGE = 1e6


def t64(v):
    return torch.tensor(v, **F64)


def rfcavity(particles, energy, mc2, n_charges, length, voltage, phase, frequency):
    """The map of the module docstring on (N, 7) particles; returns ((N, 7) particles, outgoing reference energy)."""
    q, p0c = bmadx.cheetah_to_bmad_coords(particles, energy, mc2)
    x, px, y, py, z, pz = (q[..., j] for j in range(6))
    x, y, z = bmadx.track_a_drift(length / 2, x, px, y, py, z, pz, p0c, mc2)
    pc_old = (1 + pz) * p0c
    beta_old = pc_old / (pc_old.square() + mc2.square()).sqrt()
    time = bmadx.particle_rf_time(z, pz, p0c, mc2)
    dE = abs(n_charges) * voltage * torch.sin(2 * torch.pi * (phase - frequency * time))
    E_new = pc_old / beta_old + dE
    pc = (E_new.square() - mc2.square()).sqrt()
    beta = pc / E_new
    pz = (pc - p0c) / p0c
    z = z * beta / beta_old
    x, y, z = bmadx.track_a_drift(length / 2, x, px, y, py, z, pz, p0c, mc2)
    out, ref_energy = bmadx.bmad_to_cheetah_coords(torch.stack([x, px, y, py, z, pz], dim=-1), p0c, mc2)
    return out, ref_energy


def main():
    arrays = {"frequency": np.asarray(FREQUENCY), "voltage": np.asarray(VOLTAGE)}
    g = torch.Generator().manual_seed(26)
    beams = {}
    for sp_name, E in (("electron", 1e8), ("proton", 2e9)):
        species = cheetah.Species(sp_name, **F64)
        energy = t64(E)
        arrays[f"{sp_name}_energy"] = npy(energy)
        arrays[f"{sp_name}_species"] = np.asarray(species_meta(species))
        for tag, sigma_tau in (("short", 1e-2), ("long", 1.0)):
            x = torch.randn(N, 7, generator=g, **F64) * t64([1e-3, 2e-5, 1e-3, 2e-5, sigma_tau, 2e-3, 0.0])
            x[:, 6] = 1.0
            if tag == "long":
                # the doomed row: 100 keV of kinetic energy, at f t = 0.38 (phase 0.13 - 0.38 = -0.25: the full decelerating voltage)
                p0c = (energy.square() - species.mass_eV.square()).sqrt()
                x[-1, 4] = 0.38 * 299792458.0 / FREQUENCY
                x[-1, 5] = (species.mass_eV + 1e5 - energy) / p0c
            beams[sp_name, tag] = (x, energy, species)
            arrays[f"{sp_name}_in_{tag}"] = npy(x)
            print(sp_name, tag, "rows with |f t| > 1:", int((x[:, 4].abs() * FREQUENCY / 299792458.0 > 1).sum()))
    cases = [(sp, phase, length) for sp in ("electron",) for phase in (0.0, 0.5, 0.13) for length in (0.0, 0.3)]
    cases += [("proton", 0.13, 0.0), ("proton", 0.13, 0.3), ("proton", 0.5, 0.3)]
    names = []
    for sp_name, phase, length in cases:
        name = f"{sp_name}_phase{phase:g}_L{length:g}"
        names.append(name)
        arrays[f"{name}_params"] = np.asarray([length, VOLTAGE, phase, FREQUENCY])
        arrays[f"{name}_species"] = np.asarray(sp_name)
        for tag in ("short", "long"):
            x, energy, species = beams[sp_name, tag]
            out, e_out = rfcavity(x, energy, species.mass_eV, float(species.num_elementary_charges), t64(length), t64(VOLTAGE),
                                  t64(phase), t64(FREQUENCY))
            arrays[f"{name}_{tag}_out"] = npy(out)
            arrays[f"{name}_{tag}_energy_out"] = npy(e_out)
            lost = out.isnan().any(dim=1)
            moved = float((out[~lost, 5] - x[~lost, 5]).abs().max())
            print(name, tag, "NaN rows:", lost.nonzero().flatten().tolist(), "columns:", out[lost].isnan().any(dim=0).nonzero().flatten().tolist(),
                  f"largest change of delta {moved:.2e}")
    arrays["names"] = np.asarray(names)
    arrays["beams"] = np.asarray(["short", "long"])
    save("dkd_rfcavity.npz", **arrays)


if __name__ == "__main__":
    main()
