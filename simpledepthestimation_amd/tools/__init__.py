"""Command-line tools (the reference's tools/): `python -m simpledepthestimation_amd.tools.demo`."""
