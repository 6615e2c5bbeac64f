class PyGLinkPropPredDataset:
    """A name to patch; the stand-in loads no data sets."""

    def __init__(self, *args, **kwargs):
        raise NotImplementedError('the tgb stand-in holds no data sets')
