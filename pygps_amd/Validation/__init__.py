"""``from pygps_amd.Validation import valid``: the reference keeps its validation helpers in a package of this name
(pyGPs/Validation/valid.py), and its demos import them from there; the module itself is ``pygps_amd.valid``."""
from .. import valid  # noqa: F401
