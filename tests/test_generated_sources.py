"""The generated k-loop files are what tools/gen_tile_asm.py writes: the product's tile_task_asm.inc and the probe's
tile_task_asm_probe.inc are committed, and an edit to either one or to the generator alone would go unnoticed."""
import pathlib
import subprocess
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent
COMMITTED = [ROOT / "azdopt_amd" / "csrc" / "tile_task_asm.inc", ROOT / "tools" / "probes" / "tile_task_asm_probe.inc"]


def test_generated_k_loops_match_the_generator(tmp_path):
    subprocess.run([sys.executable, str(ROOT / "tools" / "gen_tile_asm.py"), str(tmp_path)], check=True, capture_output=True)
    assert sorted(p.name for p in tmp_path.iterdir()) == sorted(p.name for p in COMMITTED)
    for committed in COMMITTED:
        assert (tmp_path / committed.name).read_bytes() == committed.read_bytes(), committed.name
