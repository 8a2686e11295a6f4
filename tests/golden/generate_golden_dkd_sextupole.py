#!/usr/bin/env python3
"""Golden vectors for the drift-kick-drift Sextupole: tests/golden/dkd_sextupole.npz.

Run in the build container only (imports the reference read-only through generate_golden.py):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/generate_golden_dkd_sextupole.py

The reference has no drift-kick-drift method for its Sextupole. Its Bmad-X module has the building blocks, and this script
composes the map from them in float64 (DATA only in the file: inputs, parameters, outputs):

    (tau, delta) -> (z, pz)                         cheetah_to_bmad_z_pz, once
    offset_particle_set(misalignment, tilt)
    track_a_drift(h),  h = L / (2 n)
    n x [ px -= (kappa / 2) (x^2 - y^2),  py += kappa x y,  kappa = k2 L / n;  track_a_drift(2 h), h behind the last kick ]
    offset_particle_unset
    (z, pz) -> (tau, delta)                         bmad_to_cheetah_z_pz, once

Cases: upright / tilted / misaligned / both, num_steps 1 and 3, on two beams of 257 electrons at 100 MeV (sigma_x = sigma_y =
1 mm and 5 mm, sigma_delta = 2e-3).
"""

import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from generate_golden import cheetah, np, npy, save, species_meta, torch  # noqa: E402

from cheetah.utils import bmadx  # noqa: E402

F64 = {"dtype": torch.float64}
N = 257


def t64(v):
    return torch.tensor(v, **F64)


def dkd_sextupole(particles, energy, mc2, length, k2, tilt, misalignment, num_steps):
    """The map of the module docstring on (N, 7) particles; returns ((N, 7) particles, outgoing reference energy)."""
    x, px, y, py, tau, delta = (particles[..., j] for j in range(6))
    z, pz, p0c = bmadx.cheetah_to_bmad_z_pz(tau, delta, energy, mc2)
    x, px, y, py = bmadx.offset_particle_set(misalignment[0], misalignment[1], tilt, x, px, y, py)
    h = length / (2 * num_steps)
    kappa = k2 * length / num_steps
    x, y, z = bmadx.track_a_drift(h, x, px, y, py, z, pz, p0c, mc2)
    for step in range(num_steps):
        px = px - 0.5 * kappa * (x.square() - y.square())
        py = py + kappa * x * y
        x, y, z = bmadx.track_a_drift(2 * h if step + 1 < num_steps else h, x, px, y, py, z, pz, p0c, mc2)
    x, px, y, py = bmadx.offset_particle_unset(misalignment[0], misalignment[1], tilt, x, px, y, py)
    tau, delta, ref_energy = bmadx.bmad_to_cheetah_z_pz(z, pz, p0c, mc2)
    return torch.stack([x, px, y, py, tau, delta, torch.ones_like(x)], dim=-1), ref_energy


def main():
    species = cheetah.Species("electron", **F64)
    energy = t64(1e8)
    arrays = {"energy": npy(energy), "species": np.asarray(species_meta(species))}
    g = torch.Generator().manual_seed(20)
    beams = {}
    for tag, sigma in (("1mm", 1e-3), ("5mm", 5e-3)):
        x = torch.randn(N, 7, generator=g, **F64) * t64([sigma, 2e-5, sigma, 2e-5, 1e-4, 2e-3, 0.0])
        x[:, 6] = 1.0
        beams[tag] = x
        arrays[f"in_{tag}"] = npy(x)
    cases = [  # name, length, k2, tilt, misalignment, num_steps
        ("upright_n1", 0.2, 100.0, 0.0, [0.0, 0.0], 1),
        ("tilted_n3", 0.2, 100.0, 0.3, [0.0, 0.0], 3),
        ("misaligned_n1", 0.25, -80.0, 0.0, [1e-3, -5e-4], 1),
        ("tilted_misaligned_n3", 0.25, -80.0, -0.4, [1e-3, -5e-4], 3),
    ]
    for name, length, k2, tilt, mis, n in cases:
        arrays[f"{name}_params"] = np.asarray([length, k2, tilt, mis[0], mis[1]])
        arrays[f"{name}_steps"] = np.asarray(n)
        for tag, x in beams.items():
            out, e_out = dkd_sextupole(x, energy, species.mass_eV, t64(length), t64(k2), t64(tilt), t64(mis), n)
            drift, _ = dkd_sextupole(x, energy, species.mass_eV, t64(length), t64(0.0), t64(tilt), t64(mis), n)
            arrays[f"{name}_{tag}_out"] = npy(out)
            arrays[f"{name}_{tag}_energy_out"] = npy(e_out)
            moved = ((out - drift).abs().amax(dim=0) / out.abs().amax(dim=0))[:4]
            print(name, tag, "the kick moves x, px, y, py by", [f"{float(m):.1e}" for m in moved], "of the column's largest magnitude")
    arrays["names"] = np.asarray([c[0] for c in cases])
    arrays["beams"] = np.asarray(list(beams))
    save("dkd_sextupole.npz", **arrays)


if __name__ == "__main__":
    main()
