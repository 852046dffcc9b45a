"""PDE problems (reference: src/pnmol/pde/__init__.py)."""

from . import examples, mixins, problems, reactions  # noqa: F401
