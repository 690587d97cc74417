"""Autoregressive DCA (arDCA) on MI355X: exact log-probabilities and ancestral sampling."""
