"""In-tree build of libmcq_hip.so (hipcc cross-compiles gfx950 without a GPU)."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
SO = os.path.join(CSRC, "libmcq_hip.so")
# the sweep and its C-ABI; the restore / checkpoint kernels; population annealing's resampling kernels; the quench; the heat-bath sweep;
# the quench of full_3d placements
SOURCES = [os.path.join(CSRC, "mcq_hip.hip"), os.path.join(CSRC, "mcq_resume.hip"), os.path.join(CSRC, "mcq_population.hip"),
           os.path.join(CSRC, "mcq_quench.hip"), os.path.join(CSRC, "mcq_heatbath.hip"), os.path.join(CSRC, "mcq_quench3d.hip")]
# the heat-bath queen sweep of full_3d placements, built into the same library.  It is listed apart: SOURCES names the six files whose
# device code earlier changes pinned (tests/test_quench3d_host.py counts them), and this file is compiled next to them, never into them
ADDED_SOURCES = [os.path.join(CSRC, "mcq_heatbath3d.hip")]
# parallel tempering of the board heat-bath sweep, one ladder per workgroup: a third list for the same reason (tests count the two above),
# compiled into the same library
TEMPER_SOURCES = [os.path.join(CSRC, "mcq_temper.hip")]
# parallel tempering of the full_3d heat-bath queen sweep, a ladder of attack fields per workgroup: a fourth list, as tests pin the
# three above; compiled into the same library
TEMPER3D_SOURCES = [os.path.join(CSRC, "mcq_temper3d.hip")]
# the pair-move quench of board placements: a fifth list, as tests pin the four above; compiled into the same library
PAIRS_SOURCES = [os.path.join(CSRC, "mcq_quench_pairs.hip")]
# basin hopping of board placements, the loop around the pair-move quench's descent and scan: a sixth list, as tests pin the five above;
# compiled into the same library
HOP_SOURCES = [os.path.join(CSRC, "mcq_hop.hip")]
# basin hopping of full_3d placements, the loop around the full_3d quench's descent on one attack field: a seventh list, as tests pin the
# six above; compiled into the same library
HOP3D_SOURCES = [os.path.join(CSRC, "mcq_hop3d.hip")]
# tabu search of board placements, a best-admissible-move walk over the table of the board hops with a stamp per entry: an eighth list,
# as tests pin the seven above; compiled into the same library
TABU_SOURCES = [os.path.join(CSRC, "mcq_tabu.hip")]
# tabu search of full_3d placements, a best-admissible-move walk over one attack field with a stamp per cell: a ninth list, as tests pin
# the eight above; compiled into the same library
TABU3D_SOURCES = [os.path.join(CSRC, "mcq_tabu3d.hip")]
# path relinking between board placements, a walk from one placement to another over the board table and the local search of the hops
# behind it: a tenth list, as tests pin the nine above; compiled into the same library
RELINK_SOURCES = [os.path.join(CSRC, "mcq_relink.hip")]
# path relinking between full_3d placements, a walk over (queen, cell) pairs on one attack field and the descent of the full_3d hops
# behind it: an eleventh list, as tests pin the ten above; compiled into the same library
RELINK3D_SOURCES = [os.path.join(CSRC, "mcq_relink3d.hip")]
# the n-fold way for board placements, rejection-free Metropolis dynamics as a weighted draw over the board table: a twelfth list, as
# tests pin the eleven above; compiled into the same library
NFOLD_SOURCES = [os.path.join(CSRC, "mcq_nfold.hip")]
# the n-fold way for full_3d placements, the same dynamics as a weighted draw over (queen, cell) pairs on one attack field: a thirteenth
# list, as tests pin the twelve above; compiled into the same library
NFOLD3D_SOURCES = [os.path.join(CSRC, "mcq_nfold3d.hip")]
# extremal optimisation of board placements, a rank draw over the local badness of the columns on the board table: a fourteenth list, as
# tests pin the thirteen above; compiled into the same library
EO_SOURCES = [os.path.join(CSRC, "mcq_eo.hip")]
# extremal optimisation of full_3d placements, a rank draw over the local badness of the queens on one attack field: a fifteenth list,
# as tests pin the fourteen above; compiled into the same library
EO3D_SOURCES = [os.path.join(CSRC, "mcq_eo3d.hip")]
# what the sources include: the C-ABI; the chain record of the sweep and the resume kernels; the attack field of the full_3d files;
# what the four files outside the sweep (the quenches and the heat baths) share beyond it; the lane helpers of the board heat-bath column
# update, which the tempered sweep shares; the board table of the pair-move quench, the board hops and the board tabu search
HEADERS = [os.path.join(os.path.dirname(HERE), "include", "mcq.h"), os.path.join(CSRC, "mcq_record.h"), os.path.join(CSRC, "mcq_field.h"),
           os.path.join(CSRC, "mcq_post.h"), os.path.join(CSRC, "mcq_columns.h"), os.path.join(CSRC, "mcq_table.h")]
HEADER = HEADERS[0]
# -ffp-contract=off: the reference's schedule / acceptance expressions are evaluated without
# fused multiply-adds (hipcc's default would contract beta_start + frac * delta into an FMA).
FLAGS = ["--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++17", "-fPIC", "-shared"]


def hipcc():
    exe = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(exe):
        raise RuntimeError("hipcc not found: cannot build libmcq_hip.so")
    return exe


def stale():
    if not os.path.exists(SO):
        return True
    t = os.path.getmtime(SO)
    if any(os.path.getmtime(f) > t for f in RELINK_SOURCES + RELINK3D_SOURCES + NFOLD_SOURCES + NFOLD3D_SOURCES + EO_SOURCES + EO3D_SOURCES):
        return True
    return any(os.path.getmtime(f) > t for f in SOURCES + ADDED_SOURCES + TEMPER_SOURCES + TEMPER3D_SOURCES + PAIRS_SOURCES + HOP_SOURCES + HOP3D_SOURCES + TABU_SOURCES + TABU3D_SOURCES + HEADERS)


def build(force=False, verbose=False):
    """Compile the HIP kernels + C-ABI for gfx950; returns the path of the shared library."""
    if not force and not stale():
        return SO
    cmd = [hipcc()] + FLAGS + ["-o", SO] + SOURCES + ADDED_SOURCES + TEMPER_SOURCES + TEMPER3D_SOURCES + PAIRS_SOURCES + HOP_SOURCES + HOP3D_SOURCES + TABU_SOURCES + TABU3D_SOURCES
    cmd += RELINK_SOURCES + RELINK3D_SOURCES + NFOLD_SOURCES + NFOLD3D_SOURCES + EO_SOURCES + EO3D_SOURCES
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed:\n" + r.stdout + r.stderr)
    if verbose:
        print(" ".join(cmd))
    return SO


if __name__ == "__main__":
    print(build(force=True, verbose=True))
