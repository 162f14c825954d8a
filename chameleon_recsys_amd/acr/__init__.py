"""Host-side mirror of the reference's ``acr_module/acr`` package: the CNN article encoder (ACR module) that produces the Article
Content Embedding matrix the NAR trainers consume."""
