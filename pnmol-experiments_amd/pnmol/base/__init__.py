"""Auxiliary pieces: IWP prior, random variables, filtering and smoothing steps (reference: src/pnmol/base/)."""

from . import iwp, kalman, rv, sqrt, stacked_ssm  # noqa: F401
