"""l3u_plugin.install(fast_validate=True) binds Trainer.validate on a reference-shaped stand-in
package (the layout of tests/test_plugin.py; the reference itself is not imported)."""
import os
import subprocess
import sys
import textwrap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "light-3d-unet-front_amd")


def _standin(tmp_path):
    base = tmp_path / "light_unet"
    (base / "models").mkdir(parents=True)
    (base / "core").mkdir()
    (base / "__init__.py").write_text("")
    (base / "utils.py").write_text("def sliding_window_inference_3d(image, model):\n    return 'reference'\n")
    (base / "models" / "__init__.py").write_text(
        "from .unet3d import Lightweight3DUNet\nfrom .losses import FocalTverskyLoss, get_loss_function\n")
    (base / "models" / "unet3d.py").write_text("class Lightweight3DUNet:\n    origin = 'reference'\n")
    (base / "models" / "metrics.py").write_text(
        "def get_connected_components(mask, min_size=0):\n    return 'reference'\n"
        "def match_components(*a, **k):\n    return 'reference'\n"
        "def calculate_lesion_metrics(*a, **k):\n    return 'reference'\n"
        "def calculate_metrics(*a, **k):\n    return 'reference'\n")
    (base / "models" / "losses.py").write_text(
        "class FocalTverskyLoss:\n    origin = 'reference'\n\n"
        "def get_loss_function(cfg):\n    return FocalTverskyLoss()\n")
    (base / "core" / "__init__.py").write_text("")
    (base / "core" / "trainer.py").write_text(
        "from light_unet.models.unet3d import Lightweight3DUNet\n"
        "from light_unet.models.losses import get_loss_function\n"
        "from light_unet.utils import sliding_window_inference_3d\n"
        "from light_unet.models.metrics import calculate_metrics\n\n"
        "class Trainer:\n"
        "    def train_epoch(self, epoch):\n        return 'reference'\n"
        "    def _train_epoch_step_based(self, epoch):\n        return 'reference'\n"
        "    def validate(self, epoch):\n        return 'reference validate'\n")


def _run(tmp_path, body):
    _standin(tmp_path)
    script = textwrap.dedent(f"""
        import importlib.util, sys
        sys.path.insert(0, {str(tmp_path)!r})
        spec = importlib.util.spec_from_file_location("l3u_plugin", {os.path.join(PKG, "l3u_plugin.py")!r})
        plug = importlib.util.module_from_spec(spec); spec.loader.exec_module(plug)
    """) + textwrap.dedent(body)
    r = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "OK" in r.stdout


def test_install_fast_validate_binds_trainer_validate(tmp_path):
    _run(tmp_path, """
        done = plug.install(fast_validate=True)
        from light_unet.core.trainer import Trainer
        assert Trainer.validate.__module__ == "l3u_amd.fast_trainer"
        assert "Trainer.validate" in done["light_unet.core.trainer"]
        # the reference validate stays reachable
        assert Trainer._l3u_reference_validate(None, 0) == "reference validate"
        # the training loops were not asked for and stay the reference's
        assert Trainer.train_epoch(None, 0) == "reference"
        # binding twice keeps the reference original
        plug.install(fast_validate=True)
        assert Trainer._l3u_reference_validate(None, 0) == "reference validate"
        assert Trainer.validate.__module__ == "l3u_amd.fast_trainer"
        # together with the fast loops
        done = plug.install(fast_step=True, fast_validate=True)
        assert Trainer.train_epoch.__module__ == "l3u_amd.fast_trainer"
        assert set(done["light_unet.core.trainer"]) >= {"Trainer.train_epoch", "Trainer.validate"}
        fast = sys.modules["l3u_amd.fast_trainer"]
        assert callable(fast.evaluate_maps)
        print("OK")
    """)


def test_install_without_the_flag_leaves_validate_alone(tmp_path):
    _run(tmp_path, """
        plug.install()
        from light_unet.core.trainer import Trainer
        assert Trainer.validate(None, 0) == "reference validate"
        assert not hasattr(Trainer, "_l3u_reference_validate")
        plug.install(fast_step=True)
        assert Trainer.validate(None, 0) == "reference validate"
        print("OK")
    """)
