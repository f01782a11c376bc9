"""User-facing programs with the interfaces of the reference's src/examples/."""
