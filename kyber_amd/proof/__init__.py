"""Host-side mirrors of the reference's ``proof`` packages over the engine."""
