"""Mirror of the reference's ``Code/whisper_testing``: ``splitting`` scores aligner TextGrids against a gold word tier."""
