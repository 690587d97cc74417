"""Hopfield-Potts DCA on MI355X (no reference counterpart)."""
