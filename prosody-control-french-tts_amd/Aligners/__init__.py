"""Drop-in mirrors of the reference's ``Code/Aligners`` modules on the hot path."""
from .CTCFA import preprocess_text, process_files, txt_to_textgrid  # noqa: F401
