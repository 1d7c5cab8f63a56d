"""Host-side mirror of the reference's ``encrypt`` packages over the batch engine (encrypt/ibe)."""
